// Poisson CPD (CP-APR) on gfx950: the damped-Newton row solver (PDNR,
// Hansen, Plantenga & Kolda 2015), one launch per mode.
//
// For output mode m and row i, with Omega_i the nonzeros whose mode-m index
// is i, pi_x the Hadamard product of the other modes' factor rows at x and
// b = (A_m diag(lambda))[i]:
//
//   m_x  = max(b . pi_x, eps_div)
//   f    = sum_c b_c - sum_x v_x log m_x
//   Phi  = sum_x (v_x / m_x) pi_x            g = 1 - Phi
//   H    = sum_x (v_x / m_x^2) pi_x pi_x^T
//
// and an inner iteration is: pass A (m, f, Phi, g, H at b), the stopping
// test, the active set, (H_ff + mu I) d_f = -g_f by Cholesky, a projected
// backtracking line search of at most LS_MAX model-value passes, and the
// trust-region update of the row's damping mu (the box in apr.py).
//
// One workgroup of NT = 256 threads (4 waves) owns one row that has
// nonzeros and runs the row's WHOLE inner loop: no relaunch, no host
// synchronisation, no atomics, a fixed summation order, so the result is
// bitwise reproducible. The host issues rows longest first.
//
// Pass A, ranks 16/32/64 (pdnr pass of MFMA_F): the row's stream range is cut
// into chunks of CH = 64 nonzeros, chunk q goes to wave q mod 4. In a wave,
// lane = k * 16 + c: nonzero k of the current group of four, columns
// blk * 16 + c of pi in NB = F/16 registers (the completion kernel's map).
//   mdl    sum over blk of b * pi, then over the 16 lanes of the group by
//          xor-shuffles 8, 4, 2, 1 (the lane groups of apr.hip with W = 16)
//   phi   += (v / mdl) pi                       f -= v log mdl
//   H     += x x^T with x = (sqrt(v) / mdl) pi as BOTH operands of
//          v_mfma_f64_16x16x4_f64 (mfma_acc.hpp), upper block pairs only
// The groups fold by xor-shuffles 16, 32; the four waves then add their
// accumulator registers into H in LDS one wave after the other (wave order,
// a barrier between two waves), and their Phi and f partials are summed in
// wave order.
// Other ranks 1..64: the workgroup stages TR = 32 nonzeros of pi in LDS,
// eight lanes per nonzero reduce the model value by xor-shuffles, and every
// thread accumulates up to PAIRS elements (i, j) of H from the tile, as
// complete_generic_kern does. Correct, not tuned.
// A line-search evaluation is the same pass without Phi and H.
//
// LDS (doubles): H[F * (F + 1)] | b[64] | b'[64] | g[64] | d[64] | Phi[64] |
// diag H[64] | per-wave Phi partials[4 * 64] | scalars[16] | generic ranks
// only: tile[TR * F] | w1[TR] | w2[TR] | fx[TR].  38.5 KB at F = 64.
//
// Barriers. The inner loop, the line search and their exits enclose
// barriers, so every such branch is decided from values that ALL threads
// read from the scalar block `sc` in LDS after a barrier, and a second
// barrier follows the reads before any thread may overwrite them; mu, f,
// alpha and the counters are then the same register value in every thread
// because they are computed from those reads alone. Loop bounds that are
// not read from LDS (F, max_inner, LS_MAX, the row's range) are kernel
// arguments or loads of one address that every thread makes. The places
// where decision values are written are marked [D1]..[D3] below.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "launchers.hpp"
#include "mfma_acc.hpp"

namespace {

constexpr int MAX_RANK = 64;
constexpr int NT = 256;        // threads per workgroup
constexpr int NW = NT / WAVE;  // waves per workgroup
constexpr int CH = 64;         // nonzeros per chunk of the MFMA pass
constexpr int TR = 32;         // nonzeros staged per LDS tile (generic pass)
constexpr int LS_MAX = 11;     // line-search evaluations per inner iteration
constexpr int VS = 64;         // stride of the vectors kept in LDS

// scalar block: [0, NW) per-wave partials of -sum v log m, then
enum {
  SC_F = 4, SC_VIOL, SC_NRM, SC_PRED, SC_BAD, SC_SLOPE, SC_SUMB, SC_N = 16
};

// non-root levels 1..NO of the stream, BY VALUE in the kernel-arg block
struct PdnrTab {
  const int32_t * idx[7];
  const double * mats[7];
};

__host__ __device__ inline int lds_doubles(int F, bool generic) {
  return F * (F + 1) + 6 * VS + NW * VS + SC_N
         + (generic ? TR * F + 3 * TR : 0);
}

template <int W>
__device__ __forceinline__ double group_sum(double x) {
  #pragma unroll
  for (int o = W >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

template <int W>
__device__ __forceinline__ double group_max(double x) {
  #pragma unroll
  for (int o = W >> 1; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

// -sum v log m of the four waves, in wave order
__device__ __forceinline__ double fold_f(const double * sc) {
  return ((sc[0] + sc[1]) + sc[2]) + sc[3];
}

// ------------------------------------------------------ pass, ranks 16/32/64
// One pass over the row [s, e) at the point bv (in LDS). FULL: leaves H in N
// (both triangles), Phi and g = 1 - Phi in LDS. Always leaves the waves'
// partials of -sum v log m in sc[0, NW). Every thread of the workgroup calls
// this; it ends with a barrier.
template <int F, int NO, bool FULL>
__device__ __forceinline__ void
mfma_pass(const PdnrTab & tab, const double * __restrict__ vals, int64_t s,
          int64_t e, const double * bv, double eps_div, double * N,
          double * sphi, double * sg, double * part, double * sc) {
  constexpr int NB = F / 16;
  constexpr int NP = NB * (NB + 1) / 2;
  constexpr int LD = F + 1;
  constexpr int U = 4;  // groups of four nonzeros in flight
  using M = MfmaAcc<double>;
  using Acc = M::type;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int w = tid / WAVE;
  const int c = lane & 15;
  const int k = lane >> 4;

  double bb[NB], phi[NB];
  #pragma unroll
  for (int b = 0; b < NB; ++b) {
    bb[b] = bv[b * 16 + c];
    phi[b] = 0.0;
  }
  Acc acc[FULL ? NP : 1];
  #pragma unroll
  for (int p = 0; p < (FULL ? NP : 1); ++p) acc[p] = Acc{};
  double facc = 0.0;

  for (int64_t c0 = s + (int64_t)w * CH; c0 < e; c0 += (int64_t)NW * CH) {
    const int64_t ce = min64(e, c0 + CH);
    for (int64_t p0 = c0; p0 < ce; p0 += 4 * U) {
      double h[U][NB];
      double v[U];
      #pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t q = p0 + u * 4 + k;
        const bool ok = q < ce;
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
        double dot = 0.0;
        #pragma unroll
        for (int b = 0; b < NB; ++b) dot += bb[b] * h[u][b];
        const double mdl = fmax(group_sum<16>(dot), eps_div);
        facc -= v[u] * log(mdl);
        if constexpr (FULL) {
          const double w1 = v[u] / mdl;
          const double sw = sqrt(v[u]) / mdl;
          double x[NB];
          #pragma unroll
          for (int b = 0; b < NB; ++b) {
            phi[b] += w1 * h[u][b];
            x[b] = sw * h[u][b];
          }
          int p = 0;
          #pragma unroll
          for (int bi = 0; bi < NB; ++bi) {
            #pragma unroll
            for (int bj = bi; bj < NB; ++bj, ++p)
              acc[p] = M::mfma(x[bi], x[bj], acc[p]);
          }
        }
      }
    }
  }
  // the four nonzero slots k fold over each other in a fixed order
  facc += __shfl_xor(facc, 16);
  facc += __shfl_xor(facc, 32);
  if (lane == 0) sc[w] = facc;
  if constexpr (FULL) {
    #pragma unroll
    for (int b = 0; b < NB; ++b) {
      phi[b] += __shfl_xor(phi[b], 16);
      phi[b] += __shfl_xor(phi[b], 32);
      if (k == 0) part[w * VS + b * 16 + c] = phi[b];
    }
    // H: wave 0 stores, waves 1.. add, one after the other
    for (int ww = 0; ww < NW; ++ww) {
      if (w == ww) {
        int p = 0;
        #pragma unroll
        for (int bi = 0; bi < NB; ++bi) {
          #pragma unroll
          for (int bj = bi; bj < NB; ++bj, ++p) {
            #pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int row = bi * 16 + M::crow(lane, i);
              const int col = bj * 16 + c;
              const double t =
                  ww == 0 ? acc[p][i] : N[row * LD + col] + acc[p][i];
              N[row * LD + col] = t;
              if (bi != bj) N[col * LD + row] = t;
            }
          }
        }
      }
      __syncthreads();
    }
    if (tid < F) {
      const double t = ((part[tid] + part[VS + tid]) + part[2 * VS + tid])
                       + part[3 * VS + tid];
      sphi[tid] = t;
      sg[tid] = 1.0 - t;
    }
  }
  __syncthreads();
}

// ------------------------------------------------------- pass, other ranks
template <int PAIRS, bool FULL>
__device__ __forceinline__ void
generic_pass(const PdnrTab & tab, int nother, const double * __restrict__ vals,
             int64_t s, int64_t e, int F, const double * bv, double eps_div,
             double * N, double * sphi, double * sg, double * sc,
             double * tile) {
  const int LD = F + 1;
  const int FF = F * F;
  double * tw1 = tile + TR * F;
  double * tw2 = tw1 + TR;
  double * tfx = tw2 + TR;
  const int tid = threadIdx.x;
  const int vr = tid >> 3;  // the tile row whose model value this lane helps
  const int vl = tid & 7;

  double acc[PAIRS];
  int pi[PAIRS], pj[PAIRS];
  #pragma unroll
  for (int q = 0; q < PAIRS; ++q) {
    const int idx = tid + q * NT;
    acc[q] = 0.0;
    pi[q] = idx < FF ? idx / F : 0;
    pj[q] = idx < FF ? idx % F : 0;
  }
  double phi = 0.0, facc = 0.0;

  for (int64_t pt = s; pt < e; pt += TR) {
    const int nr = (int)min64((int64_t)TR, e - pt);
    __syncthreads();
    for (int x = tid; x < nr * F; x += NT) {
      const int r = x / F, f = x % F;
      double hv = 1.0;
      for (int t = 0; t < nother; ++t)
        hv *= tab.mats[t][(int64_t)tab.idx[t][pt + r] * F + f];
      tile[x] = hv;
    }
    __syncthreads();
    {
      const bool rok = vr < nr;
      double dot = 0.0;
      if (rok)
        for (int f = vl; f < F; f += 8) dot += bv[f] * tile[vr * F + f];
      const double mdl = fmax(group_sum<8>(dot), eps_div);
      if (vl == 0) {
        const double v = rok ? vals[pt + vr] : 0.0;
        const double w1 = v / mdl;
        tw1[vr] = w1;
        tw2[vr] = w1 / mdl;
        tfx[vr] = v * log(mdl);
      }
    }
    __syncthreads();
    if (tid == 0)
      for (int r = 0; r < nr; ++r) facc -= tfx[r];
    if constexpr (FULL) {
      for (int r = 0; r < nr; ++r) {
        const double * row = tile + r * F;
        const double w2 = tw2[r];
        #pragma unroll
        for (int q = 0; q < PAIRS; ++q) acc[q] += w2 * row[pi[q]] * row[pj[q]];
        if (tid < F) phi += tw1[r] * row[tid];
      }
    }
  }
  if (tid < NW) sc[tid] = tid == 0 ? facc : 0.0;
  if constexpr (FULL) {
    #pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
      const int idx = tid + q * NT;
      if (idx < FF) N[pi[q] * LD + pj[q]] = acc[q];
    }
    if (tid < F) {
      sphi[tid] = phi;
      sg[tid] = 1.0 - phi;
    }
  }
  __syncthreads();
}

// --------------------------------------------------------------- the kernel
// MF = 16/32/64: the MFMA pass at that rank (NO non-root levels, PAIRS
// unused); MF = 0: the generic pass (runtime F and nother, NO unused).
template <int MF, int NO, int PAIRS>
__global__ void __launch_bounds__(NT)
pdnr_kern(const PdnrTab tab, int nother, const double * __restrict__ vals,
          const int64_t * __restrict__ rowptr,
          const int32_t * __restrict__ rows, int F, double eps_div,
          double inner_tol, int max_inner, double mu0,
          double * __restrict__ B, double * __restrict__ Phi,
          int32_t * __restrict__ iters, double * __restrict__ viol0,
          double * __restrict__ f0o, double * __restrict__ fo,
          double * __restrict__ muo, int32_t * __restrict__ nbacko,
          int32_t * __restrict__ nfailo) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int LD = F + 1;
  double * N = sm;
  double * sb = N + F * LD;
  double * sbn = sb + VS;
  double * sg = sbn + VS;
  double * sd = sg + VS;
  double * sphi = sd + VS;
  double * shd = sphi + VS;
  double * part = shd + VS;
  double * sc = part + NW * VS;
  double * tile = sc + SC_N;

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int w = tid / WAVE;
  const bool mine = tid < F;     // wave 0, lane c = column c
  const int ti = mine ? tid : 0;
  const int64_t row = rows[blockIdx.x];
  const int64_t s = rowptr[row];
  const int64_t e = rowptr[row + 1];

#define PDNR_PASS(FULL, BV)                                                  \
  do {                                                                       \
    if constexpr (MF != 0)                                                   \
      mfma_pass<(MF ? MF : 16), NO, FULL>(tab, vals, s, e, BV, eps_div, N,   \
                                          sphi, sg, part, sc);               \
    else                                                                     \
      generic_pass<PAIRS, FULL>(tab, nother, vals, s, e, F, BV, eps_div, N,  \
                                sphi, sg, sc, tile);                         \
  } while (0)

  if (mine) sb[tid] = B[row * F + tid];
  __syncthreads();

  double mu = mu0, f = 0.0, f_first = 0.0, v0 = 0.0;
  int it = 0, nback = 0, nfail = 0;
  for (int l = 1; l <= max_inner; ++l) {
    PDNR_PASS(true, sb);
    double bw = 0.0, gw = 0.0;
    if (w == 0) {
      bw = mine ? sb[tid] : 0.0;
      gw = mine ? sg[tid] : 0.0;
      const double viol = group_max<WAVE>(mine ? fabs(fmin(bw, gw)) : 0.0);
      const double t = bw - fmax(bw - gw, 0.0);
      const double nrm = group_sum<WAVE>(mine ? t * t : 0.0);
      const double sumb = group_sum<WAVE>(bw);
      if (lane == 0) {
        // [D1] the stop test's violation, with f and the active-set radius
        sc[SC_VIOL] = viol;
        sc[SC_NRM] = nrm;
        sc[SC_F] = sumb + fold_f(sc);
      }
    }
    __syncthreads();
    const double viol = sc[SC_VIOL];
    const double eps_act = fmin(1e-8, sqrt(sc[SC_NRM]));
    f = sc[SC_F];
    __syncthreads();
    it = l;
    if (l == 1) {
      v0 = viol;
      f_first = f;
    }
    if (inner_tol > 0.0 && viol < inner_tol) break;  // decided from [D1]

    // the active set; fmask is wave 0's ballot of the free columns
    bool fre = false, act = false;
    unsigned long long fmask = 0;
    if (w == 0) {
      const bool fix = mine && bw == 0.0 && gw > 0.0;
      act = mine && bw > 0.0 && bw <= eps_act && gw > 0.0;
      fre = mine && !fix && !act;
      fmask = __ballot(fre);
      if (mine) shd[tid] = N[tid * LD + tid];
    }
    // left-looking Cholesky of H_ff + mu I with the rows and columns that
    // are not free replaced by identity rows: lane i of wave 0 owns row i,
    // one barrier per column (the completion kernel's, with the masks and
    // the pivot test added). The upper triangle of N keeps H.
    bool bad = false;
    for (int j = 0; j < F; ++j) {
      if (w == 0) {
        const bool fj = (fmask >> j) & 1;
        double sj = 0.0;
        if (mine && tid >= j) {
          if (fre && fj) {
            sj = N[tid * LD + j];
            if (tid == j) sj += mu;
          } else {
            sj = tid == j ? 1.0 : 0.0;
          }
          for (int k = 0; k < j; ++k) sj -= N[tid * LD + k] * N[j * LD + k];
        }
        const double piv = __shfl(sj, j);
        bad = bad || !(piv > 0.0);  // <= 0 or NaN
        const double dd = sqrt(piv);
        if (mine && tid >= j) N[tid * LD + j] = tid == j ? dd : sj / dd;
      }
      __syncthreads();
    }
    if (w == 0) {
      // L y = -g_f, then L^T d = y; lane i carries component i
      double r = fre ? -gw : 0.0;
      for (int j = 0; j < F; ++j) {
        const double y = __shfl(r, j) / N[j * LD + j];
        if (tid == j) r = y;
        else if (mine && tid > j) r -= N[tid * LD + j] * y;
      }
      for (int j = F - 1; j >= 0; --j) {
        const double x = __shfl(r, j) / N[j * LD + j];
        if (tid == j) r = x;
        else if (tid < j) r -= N[j * LD + tid] * x;
      }
      const double df = fre ? r : 0.0;
      // (H_ff d_f)_i from the upper triangle and the saved diagonal
      double hd = 0.0;
      for (int j = 0; j < F; ++j) {
        const double dj = __shfl(df, j);
        const double hij = j == ti ? shd[ti]
                           : (j > ti ? N[ti * LD + j] : N[j * LD + ti]);
        hd += hij * dj;
      }
      const double gd = group_sum<WAVE>(fre ? gw * df : 0.0);
      const double dhd = group_sum<WAVE>(fre ? df * hd : 0.0);
      if (mine) sd[tid] = fre ? df : (act ? -gw : 0.0);
      if (lane == 0) {
        // [D2] the pivot failure, with the predicted decrease
        sc[SC_BAD] = bad ? 1.0 : 0.0;
        sc[SC_PRED] = gd + 0.5 * dhd;
      }
    }
    __syncthreads();
    const bool isbad = sc[SC_BAD] != 0.0;
    const double pred = sc[SC_PRED];
    __syncthreads();

    bool accepted = false;
    double fnew = f, alpha = 1.0;
    if (!isbad) {  // decided from [D2]
      for (int ev = 0; ev < LS_MAX; ++ev) {
        if (w == 0) {
          const double bn = mine ? fmax(bw + alpha * sd[tid], 0.0) : 0.0;
          if (mine) sbn[tid] = bn;
          const double slope = group_sum<WAVE>(mine ? gw * (bn - bw) : 0.0);
          const double sumb = group_sum<WAVE>(bn);
          if (lane == 0) {
            // [D3] the sufficient-decrease test's right-hand side; its
            // left-hand side is sc[SC_SUMB] and the waves' partials that
            // the pass below leaves in sc[0, NW)
            sc[SC_SLOPE] = slope;
            sc[SC_SUMB] = sumb;
          }
        }
        __syncthreads();
        PDNR_PASS(false, sbn);
        fnew = sc[SC_SUMB] + fold_f(sc);
        const double slope = sc[SC_SLOPE];
        __syncthreads();
        ++nback;
        if (fnew <= f + 1e-4 * slope) {  // decided from [D3]; NaN rejects
          accepted = true;
          break;
        }
        alpha *= 0.5;
      }
    }
    if (accepted) {
      const double rho = (fnew - f) / pred;
      if (pred == 0.0) mu *= 10.0;
      else if (rho < 0.25) mu *= 3.5;
      else if (rho > 0.75) mu *= 2.0 / 7.0;
      f = fnew;
      if (mine) sb[tid] = sbn[tid];
    } else {
      mu *= 10.0;
      ++nfail;
    }
    __syncthreads();
  }
#undef PDNR_PASS

  if (mine) {
    B[row * F + tid] = sb[tid];
    Phi[row * F + tid] = sphi[tid];
  }
  if (tid == 0) {
    iters[row] = it;
    viol0[row] = v0;
    f0o[row] = f_first;
    fo[row] = f;
    muo[row] = mu;
    nbacko[row] = nback;
    nfailo[row] = nfail;
  }
}

int check_lds(size_t bytes) {
  int dev = 0, lim = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  e = hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock,
                            dev);
  if (e != hipSuccess) return (int)e;
  return bytes <= (size_t)lim ? 0 : (int)hipErrorInvalidValue;
}

}  // namespace

namespace splatt {
namespace hip {

int apr_pdnr(const int32_t * const * idx, const double * const * mats,
             int nother, const double * vals, const int64_t * rowptr,
             const int32_t * rows, int64_t nrows, int F, double eps_div,
             double inner_tol, int max_inner, double mu0, double * B,
             double * Phi, int32_t * iters, double * viol0, double * f0,
             double * f, double * mu, int32_t * nback, int32_t * nfail,
             void * stream) {
  if (nrows <= 0) return 0;
  if (nother < 2 || nother > 7 || F < 1 || F > MAX_RANK || max_inner < 1
      || nrows > 0x7FFFFFFF || !(mu0 > 0.0) || !(eps_div > 0.0))
    return (int)hipErrorInvalidValue;
  PdnrTab tab{};
  for (int t = 0; t < nother; ++t) {
    tab.idx[t] = idx[t];
    tab.mats[t] = mats[t];
  }
  const bool generic = !(F == 16 || F == 32 || F == 64);
  const size_t lds = (size_t)lds_doubles(F, generic) * sizeof(double);
  if (int rc = check_lds(lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((uint32_t)nrows), block(NT);
#define PARGS tab, nother, vals, rowptr, rows, F, eps_div, inner_tol, \
              max_inner, mu0, B, Phi, iters, viol0, f0, f, mu, nback, nfail
#define PDNR_NO(MF, NO) \
  hipLaunchKernelGGL((pdnr_kern<MF, NO, 1>), grid, block, lds, st, PARGS)
#define PDNR_MF(MF)                        \
  switch (nother) {                        \
    case 2: PDNR_NO(MF, 2); break;         \
    case 3: PDNR_NO(MF, 3); break;         \
    case 4: PDNR_NO(MF, 4); break;         \
    case 5: PDNR_NO(MF, 5); break;         \
    case 6: PDNR_NO(MF, 6); break;         \
    default: PDNR_NO(MF, 7); break;        \
  }
  if (F == 16) { PDNR_MF(16) }
  else if (F == 32) { PDNR_MF(32) }
  else if (F == 64) { PDNR_MF(64) }
  else if (F * F <= NT)
    hipLaunchKernelGGL((pdnr_kern<0, 2, 1>), grid, block, lds, st, PARGS);
  else if (F * F <= 4 * NT)
    hipLaunchKernelGGL((pdnr_kern<0, 2, 4>), grid, block, lds, st, PARGS);
  else
    hipLaunchKernelGGL((pdnr_kern<0, 2, 16>), grid, block, lds, st, PARGS);
#undef PDNR_MF
#undef PDNR_NO
#undef PARGS
  return launch_rc();
}

}  // namespace hip
}  // namespace splatt
