// Fused dense tail of one ALS mode update on gfx950 (f64, ranks 16/32/64).
//
// Given the MTTKRP output K (n x F) and Ginv (F x F), steady-state max-norm:
//
//   T = K @ Ginv ;  lam[f] = max(1, max_i |T[i,f]|) ;  A = T / lam
//   gram = A^T A ;  inner[f] = sum_i K[i,f] * A[i,f]   (on request)
//
// in two launches that make three passes over an n x F array (read K, read
// K, write A) where the library chain (mm, abs, amax, div_, gram, and mul +
// sum for the fit) makes twelve:
//
//   pass 1  reads K, forms T in registers and reduces the column maxima of
//           |T| into lam with an integer atomicMax on the bit pattern
//           (non-negative doubles order like their bits; a NaN is the
//           largest, as amax propagates it). lam starts at 1.0, so the
//           clamp is part of the maximum. Nothing n x F is written.
//   pass 2  reads K again, recomputes T with the same device function —
//           the same bits, so the largest entry of a scaled column is
//           exactly 1 — divides (IEEE division), stores A, and accumulates
//           A^T A and, when asked, inner.
//
// Recomputing T costs n F^2 FMAs on the matrix cores; storing it in pass 1
// and rescaling it in place would cost a fourth pass over memory.
//
// lam, gram and inner must hold 1, 0 and 0 when pass 1 starts: the
// Hadamard + inverse launch in front (splatt::hip::als_prep,
// dense_kernels.hip) resets them, so there is no memset launch.
//
// Layout. A wave owns 16 rows per step; T = K * Ginv is a plain (not
// transposed) v_mfma_f64_16x16x4_f64 product per 16-column block:
//   A operand  [m = lane&15][k = lane>>4] = K[row m][sigma(j, k)]
//   B operand  [k = lane>>4][n = lane&15] = Ginv[sigma(j, k)][16cb + n]
//   C/D        reg i of lane (q = lane>>4, c = lane&15) = T[q + 4i][16cb + c]
// The contraction index may be permuted freely as long as both operands
// agree: sigma(j, q) = 8*(j/2) + 2q + j%2 lets a lane fetch K as 16-B
// loads, four lanes covering 64 contiguous bytes of a row. The C/D layout
// is at once the store layout (reg i: four whole rows of a column block,
// contiguous) and the operand layout of the self-transpose Gram trick of
// gram_mfma_kern (mfma_acc.hpp): reg i holds 4 rows x 16 columns, fed as
// both operands it adds those rows' outer products to a Gram tile.
// Ginv operands stay in registers at ranks 16/32 and are re-read from LDS
// at rank 64 (64 doubles a lane otherwise).
//
// The four waves of a block fold their Gram tiles, inner sums and column
// maxima through LDS; one atomic per element per block reaches memory.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "launchers.hpp"
#include "mfma_acc.hpp"

namespace {

constexpr int NT = 256;
constexpr int WPB = NT / WAVE;
constexpr int TILE = 16;         // rows per wave step
constexpr int MAX_BLOCKS = 2048;

using M = MfmaAcc<double>;
using Acc = M::type;
using D2 = __attribute__((ext_vector_type(2))) double;

template <int F>
struct Shape {
  static constexpr int J = F / 4;             // K=4 chunks of the contraction
  static constexpr int NB = F / 16;           // 16-wide column blocks
  static constexpr int NP = NB * (NB + 1) / 2;
  static constexpr bool GREG = F <= 32;       // Ginv operands in registers
};

__device__ __forceinline__ int sigma(int j, int q) {
  return 8 * (j >> 1) + 2 * q + (j & 1);
}

// B operands of every (column block, chunk) for this lane
template <int F>
__device__ __forceinline__ void load_ginv(const double * __restrict__ Ginv,
                                          int q, int c,
                                          double (&Gb)[Shape<F>::NB][Shape<F>::J]) {
  #pragma unroll
  for (int cb = 0; cb < Shape<F>::NB; ++cb) {
    #pragma unroll
    for (int j = 0; j < Shape<F>::J; ++j)
      Gb[cb][j] = Ginv[sigma(j, q) * F + 16 * cb + c];
  }
}

// T tile of rows r0 .. r0+15 (rows past n read as zero). Both passes call
// this, so they see identical bits. Gl: Ginv in LDS (rank 64 only).
template <int F>
__device__ __forceinline__ void tile_T(
    const double * __restrict__ K, int64_t n, int64_t r0, int q, int c,
    const double (&Gb)[Shape<F>::NB][Shape<F>::J], const double * Gl,
    Acc (&T)[Shape<F>::NB]) {
  constexpr int J = Shape<F>::J, NB = Shape<F>::NB;
  double a[J];
  const int64_t row = r0 + c;
  if (row < n) {
    const D2 * p = reinterpret_cast<const D2 *>(K + row * F + 2 * q);
    #pragma unroll
    for (int jj = 0; jj < J / 2; ++jj) {
      const D2 v = p[4 * jj];
      a[2 * jj] = v.x;
      a[2 * jj + 1] = v.y;
    }
  } else {
    #pragma unroll
    for (int j = 0; j < J; ++j) a[j] = 0.0;
  }
  #pragma unroll
  for (int cb = 0; cb < NB; ++cb) {
    Acc acc = Acc{};
    #pragma unroll
    for (int j = 0; j < J; ++j) {
      double b;
      if constexpr (Shape<F>::GREG) b = Gb[cb][j];
      else b = Gl[sigma(j, q) * F + 16 * cb + c];
      acc = M::mfma(a[j], b, acc);
    }
    T[cb] = acc;
  }
}

__device__ __forceinline__ unsigned long long umax64(unsigned long long a,
                                                     unsigned long long b) {
  return a > b ? a : b;
}

constexpr unsigned long long ONE_BITS = 0x3FF0000000000000ull;

// ------------------------------------------------------------------ pass 1
template <int F>
__global__ void __launch_bounds__(NT)
tail_max_kern(const double * __restrict__ K, const double * __restrict__ Ginv,
              int64_t n, unsigned long long * __restrict__ lam_bits) {
  constexpr int NB = Shape<F>::NB;
  __shared__ double Gl[Shape<F>::GREG ? 1 : F * F];
  __shared__ unsigned long long red[WPB * F];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wv = tid >> 6;
  const int q = lane >> 4, c = lane & 15;

  double Gb[NB][Shape<F>::J];
  if constexpr (Shape<F>::GREG) {
    load_ginv<F>(Ginv, q, c, Gb);
  } else {
    for (int e = tid; e < F * F; e += NT) Gl[e] = Ginv[e];
    __syncthreads();
  }

  unsigned long long mx[NB];
  #pragma unroll
  for (int cb = 0; cb < NB; ++cb) mx[cb] = 0;

  const int64_t ntiles = (n + TILE - 1) / TILE;
  for (int64_t t = (int64_t)blockIdx.x * WPB + wv; t < ntiles;
       t += (int64_t)gridDim.x * WPB) {
    Acc T[NB];
    tile_T<F>(K, n, t * TILE, q, c, Gb, Gl, T);
    #pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      #pragma unroll
      for (int i = 0; i < 4; ++i)
        mx[cb] = umax64(mx[cb],
                        (unsigned long long)__double_as_longlong(fabs(T[cb][i])));
    }
  }
  #pragma unroll
  for (int cb = 0; cb < NB; ++cb) {
    mx[cb] = umax64(mx[cb], __shfl_xor(mx[cb], 16, WAVE));
    mx[cb] = umax64(mx[cb], __shfl_xor(mx[cb], 32, WAVE));
    if (q == 0) red[wv * F + 16 * cb + c] = mx[cb];
  }
  __syncthreads();
  if (tid < F) {
    unsigned long long m = red[tid];
    #pragma unroll
    for (int w = 1; w < WPB; ++w) m = umax64(m, red[w * F + tid]);
    if (m > ONE_BITS) atomicMax(&lam_bits[tid], m);   // lam starts at 1.0
  }
}

// ------------------------------------------------------------------ pass 2
template <int F, bool INNER>
__global__ void __launch_bounds__(NT)
tail_scale_kern(const double * __restrict__ K,
                const double * __restrict__ Ginv,
                const double * __restrict__ lam, int64_t n,
                double * __restrict__ A, double * __restrict__ gram,
                double * __restrict__ inner) {
  constexpr int NB = Shape<F>::NB, NP = Shape<F>::NP;
  // Ginv operands at rank 64, then the block's Gram fold
  __shared__ double sm[F * F];
  __shared__ double red[INNER ? WPB * F : 1];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wv = tid >> 6;
  const int q = lane >> 4, c = lane & 15;

  double Gb[NB][Shape<F>::J];
  if constexpr (Shape<F>::GREG) {
    load_ginv<F>(Ginv, q, c, Gb);
  } else {
    for (int e = tid; e < F * F; e += NT) sm[e] = Ginv[e];
    __syncthreads();
  }
  double lamr[NB];
  #pragma unroll
  for (int cb = 0; cb < NB; ++cb) lamr[cb] = lam[16 * cb + c];

  Acc g[NP];
  #pragma unroll
  for (int p = 0; p < NP; ++p) g[p] = Acc{};
  double in[NB];
  #pragma unroll
  for (int cb = 0; cb < NB; ++cb) in[cb] = 0.0;

  const int64_t ntiles = (n + TILE - 1) / TILE;
  for (int64_t t = (int64_t)blockIdx.x * WPB + wv; t < ntiles;
       t += (int64_t)gridDim.x * WPB) {
    const int64_t r0 = t * TILE;
    Acc T[NB];
    tile_T<F>(K, n, r0, q, c, Gb, sm, T);
    // rows past n hold T = 0, so A = 0 / lam adds nothing to the Gram
    #pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double a = T[cb][i] / lamr[cb];
        T[cb][i] = a;
        const int64_t row = r0 + M::crow(lane, i);
        if (row < n) {
          const int64_t off = row * F + 16 * cb + c;
          if constexpr (INNER) in[cb] += K[off] * a;
          A[off] = a;
        }
      }
    }
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      int p = 0;
      #pragma unroll
      for (int bi = 0; bi < NB; ++bi) {
        #pragma unroll
        for (int bj = bi; bj < NB; ++bj, ++p)
          g[p] = M::mfma(T[bi][i], T[bj][i], g[p]);
      }
    }
  }

  // fold the four waves' Gram tiles in LDS (upper block triangle), wave by
  // wave, then one atomic per element per block
  __syncthreads();                       // rank 64: Ginv reads are done
  for (int w = 0; w < WPB; ++w) {
    if (wv == w) {
      int p = 0;
      #pragma unroll
      for (int bi = 0; bi < NB; ++bi) {
        #pragma unroll
        for (int bj = bi; bj < NB; ++bj, ++p) {
          #pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int e = (16 * bi + M::crow(lane, i)) * F + 16 * bj + c;
            sm[e] = w == 0 ? g[p][i] : sm[e] + g[p][i];
          }
        }
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < F * F; e += NT) {
    const int r = e / F, cc = e % F;
    const double v = (r >> 4) <= (cc >> 4) ? sm[e] : sm[cc * F + r];
    unsafeAtomicAdd(&gram[e], v);
  }
  if constexpr (INNER) {
    #pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      double s = in[cb];
      s += __shfl_xor(s, 16, WAVE);
      s += __shfl_xor(s, 32, WAVE);
      if (q == 0) red[wv * F + 16 * cb + c] = s;
    }
    __syncthreads();
    if (tid < F) {
      double s = red[tid];
      #pragma unroll
      for (int w = 1; w < WPB; ++w) s += red[w * F + tid];
      unsafeAtomicAdd(&inner[tid], s);
    }
  }
}

template <int F>
int launch_tail(const double * K, const double * Ginv, int64_t n, double * A,
                double * lam, double * gram, double * inner, hipStream_t st) {
  const int64_t ntiles = (n + TILE - 1) / TILE;
  int64_t nblocks = (ntiles + WPB - 1) / WPB;
  if (nblocks > MAX_BLOCKS) nblocks = MAX_BLOCKS;
  dim3 grid((uint32_t)nblocks), block(NT);
  hipLaunchKernelGGL((tail_max_kern<F>), grid, block, 0, st, K, Ginv, n,
                     reinterpret_cast<unsigned long long *>(lam));
  if (inner)
    hipLaunchKernelGGL((tail_scale_kern<F, true>), grid, block, 0, st, K,
                       Ginv, lam, n, A, gram, inner);
  else
    hipLaunchKernelGGL((tail_scale_kern<F, false>), grid, block, 0, st, K,
                       Ginv, lam, n, A, gram, inner);
  return launch_rc();
}

}  // namespace

namespace splatt {
namespace hip {

// (tests cover launches past the cap)
int64_t als_tail_cap_rows() { return (int64_t)MAX_BLOCKS * WPB * TILE; }

int als_tail(const double * K, const double * Ginv, int64_t n, int F,
             double * A, double * lam, double * gram, double * inner,
             void * stream) {
  if (((uintptr_t)K | (uintptr_t)A) & 15) return -2;
  if (n <= 0) return (F == 16 || F == 32 || F == 64) ? 0 : -1;
  hipStream_t st = (hipStream_t)stream;
  switch (F) {
    case 16: return launch_tail<16>(K, Ginv, n, A, lam, gram, inner, st);
    case 32: return launch_tail<32>(K, Ginv, n, A, lam, gram, inner, st);
    case 64: return launch_tail<64>(K, Ginv, n, A, lam, gram, inner, st);
    default: return -1;
  }
}

}  // namespace hip
}  // namespace splatt
