// Tensor completion (observed-entries ALS) on gfx950.
//
// Row-wise update for output mode m: for every row i with observed entries
// Omega_i and h_x = hadamard_{t != m} A_t[i_t(x), :],
//
//   A_m[i,:] = (sum_x h_x h_x^T + reg*I)^-1 * sum_x val_x * h_x
//
// The mode's root-sorted stream makes every Omega_i a contiguous range, cut
// on the host into segments of bounded nnz that never cross a row. One
// workgroup owns one segment:
//   * F in {16,32,64}: a single wave folds four nonzeros per
//     v_mfma_f64_16x16x4_f64 into the upper 16x16 block pairs of sum h h^T
//     (the self-transpose operand trick of gram_mfma_kern) and keeps the
//     right-hand side lane-wise.
//   * other ranks 1..64: 256 threads, one per (i,j) element, LDS-staged
//     outer products like gram_kern. Correct, not tuned.
// A row that fits one segment is finished in place: reg on the diagonal,
// Cholesky in LDS, two triangular solves, one plain row store. A row that
// spans several segments parks its partials in a workspace slot per
// segment; complete_reduce_kern folds the slots in order and solves. No
// atomics anywhere, so the update is run-to-run reproducible.
//
// With reg > 0 every system is SPD: no jitter escalation.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "launchers.hpp"
#include "mfma_acc.hpp"

namespace {

constexpr int TR = 32;  // nonzeros staged per LDS tile (generic kernel)

// other-mode index streams + factors, BY VALUE in the kernel-arg block
struct CmplTab {
  const int32_t * idx[8];
  const double * mats[8];
};

struct PredTab {
  const int64_t * inds[8];
  const double * mats[8];
};

// workspace doubles per segment slot: the MFMA kernel parks its accumulator
// registers as they are ([pair][reg][lane]) + F rhs values; the generic
// kernel parks the full F x F matrix + F rhs values
__host__ __device__ constexpr int mfma_pairs(int F) {
  return (F / 16) * (F / 16 + 1) / 2;
}
__host__ __device__ inline int64_t slot_elems(int F) {
  if (F == 16 || F == 32 || F == 64) return mfma_pairs(F) * 256 + F;
  return (int64_t)F * F + F;
}

// Solve (N + reg*I) a = b for one row and store it. N is a full symmetric
// F x F matrix in LDS with row stride LD (the lower triangle is overwritten
// by the Cholesky factor); lane i < F of wave 0 passes b_i in `rb`. EVERY
// thread of the workgroup must call this (it contains barriers); the caller
// has synchronised after filling N.
__device__ __forceinline__ void chol_solve_store(double * N, int F, int LD,
                                                 double reg, double rb,
                                                 double * __restrict__ orow) {
  const int tid = threadIdx.x;
  const bool mine = tid < F;
  // left-looking Cholesky: lane i owns row i; one barrier per column
  for (int j = 0; j < F; ++j) {
    double s = 0.0;
    if (mine && tid >= j) {
      s = N[tid * LD + j];
      if (tid == j) s += reg;
      for (int k = 0; k < j; ++k) s -= N[tid * LD + k] * N[j * LD + k];
    }
    const double d = sqrt(__shfl(s, j));
    if (mine && tid >= j) N[tid * LD + j] = (tid == j) ? d : s / d;
    __syncthreads();
  }
  // L y = b, then L^T x = y; lane i carries component i
  double b = rb;
  for (int j = 0; j < F; ++j) {
    const double y = __shfl(b, j) / N[j * LD + j];
    if (tid == j) b = y;
    else if (mine && tid > j) b -= N[tid * LD + j] * y;
  }
  for (int j = F - 1; j >= 0; --j) {
    const double x = __shfl(b, j) / N[j * LD + j];
    if (tid == j) b = x;
    else if (tid < j) b -= N[j * LD + tid] * x;
  }
  if (mine) orow[tid] = b;
}

// ---------------------------------------------------------- MFMA segments
// One wave per segment. Lane (k = lane>>4, c = lane&15) holds h of nonzero
// k of the current group of four, column b*16+c, and feeds it as both MFMA
// operands. The K-tail of a segment whose nnz is no multiple of 4 is
// zero-filled (loads are clamped to the segment's first nonzero).
template <int F, int NO>
__global__ void __launch_bounds__(WAVE)
complete_mfma_kern(const CmplTab tab, const double * __restrict__ vals,
                   const int64_t * __restrict__ seg_start,
                   const int32_t * __restrict__ seg_len,
                   const int32_t * __restrict__ seg_row,
                   const int32_t * __restrict__ seg_slot,
                   int64_t seg0, int64_t slot0, double reg,
                   double * __restrict__ ws, double * __restrict__ out) {
  constexpr int NB = F / 16;
  constexpr int NP = NB * (NB + 1) / 2;
  constexpr int LD = F + 1;
  constexpr int U = 4;  // groups of four nonzeros in flight per iteration
  using M = MfmaAcc<double>;
  using Acc = M::type;
  extern __shared__ double sm[];  // N[F*LD] | rhs[F]

  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int k = lane >> 4;
  const int64_t sg = seg0 + blockIdx.x;
  const int64_t s = seg_start[sg];
  const int64_t e = s + seg_len[sg];

  Acc acc[NP];
  #pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = Acc{};
  double rhs[NB];
  #pragma unroll
  for (int b = 0; b < NB; ++b) rhs[b] = 0.0;

  for (int64_t p0 = s; p0 < e; p0 += 4 * U) {
    double h[U][NB];
    double v[U];
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t q = p0 + u * 4 + k;
      const bool ok = q < e;
      const int64_t qq = ok ? q : s;
      int64_t r[NO];
      #pragma unroll
      for (int t = 0; t < NO; ++t) r[t] = (int64_t)tab.idx[t][qq] * F + c;
      v[u] = ok ? vals[qq] : 0.0;
      #pragma unroll
      for (int b = 0; b < NB; ++b) {
        double x = tab.mats[0][r[0] + b * 16];
        #pragma unroll
        for (int t = 1; t < NO; ++t) x *= tab.mats[t][r[t] + b * 16];
        h[u][b] = ok ? x : 0.0;
      }
    }
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      #pragma unroll
      for (int b = 0; b < NB; ++b) rhs[b] += v[u] * h[u][b];
      int p = 0;
      #pragma unroll
      for (int bi = 0; bi < NB; ++bi) {
        #pragma unroll
        for (int bj = bi; bj < NB; ++bj, ++p)
          acc[p] = M::mfma(h[u][bi], h[u][bj], acc[p]);
      }
    }
  }
  // fold the right-hand side over the four nonzero slots k
  #pragma unroll
  for (int b = 0; b < NB; ++b) {
    rhs[b] += __shfl_xor(rhs[b], 16);
    rhs[b] += __shfl_xor(rhs[b], 32);
  }

  const int32_t slot = seg_slot[sg];
  if (slot >= 0) {
    // the row spans several segments: park the partial, registers as-is
    double * w = ws + ((int64_t)slot - slot0) * (NP * 256 + F);
    #pragma unroll
    for (int p = 0; p < NP; ++p) {
      #pragma unroll
      for (int i = 0; i < 4; ++i) w[(p * 4 + i) * WAVE + lane] = acc[p][i];
    }
    if (k == 0) {
      #pragma unroll
      for (int b = 0; b < NB; ++b) w[NP * 256 + b * 16 + c] = rhs[b];
    }
    return;
  }

  // whole row in this segment: finish it here
  {
    int p = 0;
    #pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
      #pragma unroll
      for (int bj = bi; bj < NB; ++bj, ++p) {
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = bi * 16 + M::crow(lane, i);
          const int col = bj * 16 + c;
          sm[row * LD + col] = acc[p][i];
          if (bi != bj) sm[col * LD + row] = acc[p][i];
        }
      }
    }
  }
  if (k == 0) {
    #pragma unroll
    for (int b = 0; b < NB; ++b) sm[F * LD + b * 16 + c] = rhs[b];
  }
  __syncthreads();
  const double rb = lane < F ? sm[F * LD + lane] : 0.0;
  chol_solve_store(sm, F, LD, reg, rb, out + (int64_t)seg_row[sg] * F);
}

// ------------------------------------------------------- generic segments
// 256 threads per segment, thread -> up to PAIRS (i,j) elements.
template <int PAIRS>
__global__ void __launch_bounds__(256)
complete_generic_kern(const CmplTab tab, int nother,
                      const double * __restrict__ vals,
                      const int64_t * __restrict__ seg_start,
                      const int32_t * __restrict__ seg_len,
                      const int32_t * __restrict__ seg_row,
                      const int32_t * __restrict__ seg_slot,
                      int64_t seg0, int64_t slot0, int F, double reg,
                      double * __restrict__ ws, double * __restrict__ out) {
  extern __shared__ double sm[];  // N[F*LD] | tile[TR*F] | tv[TR]
  const int LD = F + 1;
  const int FF = F * F;
  double * tile = sm + F * LD;
  double * tv = tile + TR * F;
  const int tid = threadIdx.x;
  const int64_t sg = seg0 + blockIdx.x;
  const int64_t s = seg_start[sg];
  const int64_t e = s + seg_len[sg];

  double acc[PAIRS];
  int pi[PAIRS], pj[PAIRS];
  #pragma unroll
  for (int q = 0; q < PAIRS; ++q) {
    const int idx = tid + q * 256;
    acc[q] = 0.0;
    pi[q] = idx < FF ? idx / F : 0;
    pj[q] = idx < FF ? idx % F : 0;
  }
  double rb = 0.0;

  for (int64_t pt = s; pt < e; pt += TR) {
    const int nr = (int)min((int64_t)TR, e - pt);
    __syncthreads();
    for (int x = tid; x < nr * F; x += 256) {
      const int r = x / F, f = x % F;
      double hv = 1.0;
      for (int t = 0; t < nother; ++t)
        hv *= tab.mats[t][(int64_t)tab.idx[t][pt + r] * F + f];
      tile[x] = hv;
    }
    if (tid < nr) tv[tid] = vals[pt + tid];
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const double * row = tile + r * F;
      #pragma unroll
      for (int q = 0; q < PAIRS; ++q) acc[q] += row[pi[q]] * row[pj[q]];
      if (tid < F) rb += tv[r] * row[tid];
    }
  }

  const int32_t slot = seg_slot[sg];
  if (slot >= 0) {
    double * w = ws + ((int64_t)slot - slot0) * (FF + F);
    #pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
      const int idx = tid + q * 256;
      if (idx < FF) w[idx] = acc[q];
    }
    if (tid < F) w[FF + tid] = rb;
    return;
  }
  #pragma unroll
  for (int q = 0; q < PAIRS; ++q) {
    const int idx = tid + q * 256;
    if (idx < FF) sm[pi[q] * LD + pj[q]] = acc[q];
  }
  __syncthreads();
  chol_solve_store(sm, F, LD, reg, rb, out + (int64_t)seg_row[sg] * F);
}

// ------------------------------------------------ multi-segment row solve
// One workgroup per row that spans several segments: fold its slots in
// stream order (fixed order -> reproducible), rebuild N in LDS, solve.
// MF = 16/32/64: slots are in the MFMA register layout; MF = 0: plain F x F.
template <int MF>
__global__ void __launch_bounds__(256)
complete_reduce_kern(const double * __restrict__ ws,
                     const int32_t * __restrict__ mrow,
                     const int64_t * __restrict__ mslot,
                     int64_t m0, int64_t slot0, int F, double reg,
                     double * __restrict__ out) {
  extern __shared__ double sm[];  // N[F*LD] | rhs[F]
  const int LD = F + 1;
  const int tid = threadIdx.x;
  const int64_t m = m0 + blockIdx.x;
  const int64_t a = mslot[m] - slot0;
  const int64_t b = mslot[m + 1] - slot0;
  const int NN = MF ? mfma_pairs(MF) * 256 : F * F;
  const int S = NN + F;

  for (int el = tid; el < S; el += 256) {
    double sum = 0.0;
    for (int64_t sl = a; sl < b; ++sl) sum += ws[sl * S + el];
    if (el >= NN) {
      sm[F * LD + (el - NN)] = sum;
    } else if (MF) {
      constexpr int NB = MF ? MF / 16 : 1;
      const int p = el >> 8, i = (el >> 6) & 3, lane = el & 63;
      int bi = 0, bj = 0, q = 0;
      for (int x = 0; x < NB; ++x)
        for (int y = x; y < NB; ++y, ++q)
          if (q == p) { bi = x; bj = y; }
      const int row = bi * 16 + MfmaAcc<double>::crow(lane, i);
      const int col = bj * 16 + (lane & 15);
      sm[row * LD + col] = sum;
      if (bi != bj) sm[col * LD + row] = sum;
    } else {
      sm[(el / F) * LD + el % F] = sum;
    }
  }
  __syncthreads();
  const double rb = tid < F ? sm[F * LD + tid] : 0.0;
  chol_solve_store(sm, F, LD, reg, rb, out + (int64_t)mrow[m] * F);
}

// --------------------------------------------------------- model evaluate
// predict[p] = sum_f lam_f * prod_t A_t[inds[t][p], f]. A wave takes 64
// consecutive entries: one coalesced index load per mode, then W lanes per
// entry (W = pow2 >= min(F,64), strided over f beyond W) and a shuffle
// reduce.
__global__ void __launch_bounds__(256)
kruskal_predict_kern(const PredTab tab, int nmodes,
                     const double * __restrict__ lam, int64_t n, int F,
                     int W, double * __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / WAVE);
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x / WAVE)
                      + threadIdx.x / WAVE;
  const int epr = WAVE / W;  // entries per round
  const int l = lane % W;
  for (int64_t base = wid * WAVE; base < n; base += nwaves * WAVE) {
    const int64_t pp = min(base + lane, n - 1);
    int64_t my[8];
    #pragma unroll
    for (int t = 0; t < 8; ++t) my[t] = t < nmodes ? tab.inds[t][pp] : 0;
    for (int r = 0; r < W; ++r) {
      const int el = r * epr + lane / W;
      int64_t row[8];
      #pragma unroll
      for (int t = 0; t < 8; ++t) row[t] = __shfl(my[t], el);
      double sum = 0.0;
      for (int f = l; f < F; f += W) {
        double x = lam ? lam[f] : 1.0;
        #pragma unroll
        for (int t = 0; t < 8; ++t)
          if (t < nmodes) x *= tab.mats[t][row[t] * F + f];
        sum += x;
      }
      for (int o = W >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      if (l == 0 && base + el < n) out[base + el] = sum;
    }
  }
}

// ---------------------------------------------------------------- launchers
// every launch: dynamic-LDS request checked against the device limit,
// hipGetLastError checked afterwards; nonzero return = hipError_t
int check_lds(size_t bytes) {
  int dev = 0, lim = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  e = hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock,
                            dev);
  if (e != hipSuccess) return (int)e;
  return bytes <= (size_t)lim ? 0 : (int)hipErrorInvalidValue;
}

template <int F>
int launch_mfma(const CmplTab & tab, int nother, const double * vals,
                const int64_t * seg_start, const int32_t * seg_len,
                const int32_t * seg_row, const int32_t * seg_slot,
                int64_t seg0, int64_t nseg, int64_t slot0, double reg,
                double * ws, double * out, hipStream_t st) {
  const size_t lds = ((size_t)F * (F + 1) + F) * sizeof(double);
  if (int rc = check_lds(lds)) return rc;
  dim3 grid((uint32_t)nseg), block(WAVE);
#define CARGS tab, vals, seg_start, seg_len, seg_row, seg_slot, seg0, slot0, \
              reg, ws, out
  switch (nother) {
    case 2: hipLaunchKernelGGL((complete_mfma_kern<F, 2>), grid, block, lds, st, CARGS); break;
    case 3: hipLaunchKernelGGL((complete_mfma_kern<F, 3>), grid, block, lds, st, CARGS); break;
    case 4: hipLaunchKernelGGL((complete_mfma_kern<F, 4>), grid, block, lds, st, CARGS); break;
    case 5: hipLaunchKernelGGL((complete_mfma_kern<F, 5>), grid, block, lds, st, CARGS); break;
    case 6: hipLaunchKernelGGL((complete_mfma_kern<F, 6>), grid, block, lds, st, CARGS); break;
    default: hipLaunchKernelGGL((complete_mfma_kern<F, 7>), grid, block, lds, st, CARGS); break;
  }
#undef CARGS
  return launch_rc();
}

}  // namespace

namespace splatt {
namespace hip {

int64_t complete_slot_elems(int F) { return slot_elems(F); }

int complete_segments(const int32_t * const * idx,
                      const double * const * mats, int nother,
                      const double * vals, const int64_t * seg_start,
                      const int32_t * seg_len, const int32_t * seg_row,
                      const int32_t * seg_slot, int64_t seg0, int64_t nseg,
                      int64_t slot0, int F, double reg, double * ws,
                      double * out, void * stream) {
  if (nseg <= 0) return 0;
  if (F < 1 || F > 64 || nother < 2 || nother > 7 || nseg > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  CmplTab tab{};
  for (int t = 0; t < nother; ++t) { tab.idx[t] = idx[t]; tab.mats[t] = mats[t]; }
#define MARGS tab, nother, vals, seg_start, seg_len, seg_row, seg_slot, seg0, \
              nseg, slot0, reg, ws, out, st
  if (F == 16) return launch_mfma<16>(MARGS);
  if (F == 32) return launch_mfma<32>(MARGS);
  if (F == 64) return launch_mfma<64>(MARGS);
#undef MARGS
  const size_t lds = ((size_t)F * (F + 1) + (size_t)TR * F + TR)
                     * sizeof(double);
  if (int rc = check_lds(lds)) return rc;
  dim3 grid((uint32_t)nseg), block(256);
#define GARGS tab, nother, vals, seg_start, seg_len, seg_row, seg_slot, seg0, \
              slot0, F, reg, ws, out
  const int ff = F * F;
  if (ff <= 256)
    hipLaunchKernelGGL((complete_generic_kern<1>), grid, block, lds, st, GARGS);
  else if (ff <= 1024)
    hipLaunchKernelGGL((complete_generic_kern<4>), grid, block, lds, st, GARGS);
  else
    hipLaunchKernelGGL((complete_generic_kern<16>), grid, block, lds, st, GARGS);
#undef GARGS
  return launch_rc();
}

int complete_reduce(const double * ws, const int32_t * mrow,
                    const int64_t * mslot, int64_t m0, int64_t nm,
                    int64_t slot0, int F, double reg, double * out,
                    void * stream) {
  if (nm <= 0) return 0;
  if (F < 1 || F > 64 || nm > 0x7FFFFFFF) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = ((size_t)F * (F + 1) + F) * sizeof(double);
  if (int rc = check_lds(lds)) return rc;
  dim3 grid((uint32_t)nm), block(256);
#define RARGS ws, mrow, mslot, m0, slot0, F, reg, out
  switch (F) {
    case 16: hipLaunchKernelGGL((complete_reduce_kern<16>), grid, block, lds, st, RARGS); break;
    case 32: hipLaunchKernelGGL((complete_reduce_kern<32>), grid, block, lds, st, RARGS); break;
    case 64: hipLaunchKernelGGL((complete_reduce_kern<64>), grid, block, lds, st, RARGS); break;
    default: hipLaunchKernelGGL((complete_reduce_kern<0>), grid, block, lds, st, RARGS); break;
  }
#undef RARGS
  return launch_rc();
}

int kruskal_predict(const int64_t * const * inds, const double * const * mats,
                    int nmodes, const double * lam, int64_t n, int F,
                    double * out, void * stream) {
  if (n <= 0) return 0;
  if (F < 1 || nmodes < 1 || nmodes > 8) return (int)hipErrorInvalidValue;
  PredTab tab{};
  for (int t = 0; t < nmodes; ++t) { tab.inds[t] = inds[t]; tab.mats[t] = mats[t]; }
  int W = 1;
  while (W < F && W < WAVE) W <<= 1;
  int64_t nblocks = (n + 255) / 256;
  if (nblocks > 8192) nblocks = 8192;  // grid-stride beyond this
  hipLaunchKernelGGL(kruskal_predict_kern, dim3((uint32_t)nblocks), dim3(256),
                     0, (hipStream_t)stream, tab, nmodes, lam, n, F, W, out);
  return launch_rc();
}

}  // namespace hip
}  // namespace splatt
