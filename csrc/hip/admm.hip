// Constrained CPD (AO-ADMM): the fused block-ADMM factor update on gfx950.
//
// For one output mode the driver hands over K = MTTKRP (n x F), the F x F
// matrix Ginv = (G + rho*I)^-1, the factor H and its scaled dual U. Rows
// are cut into blocks of 64; one workgroup owns one block and runs the
// whole inner loop on it
//
//   Ht = (K + rho*(H + U)) @ Ginv ;  H' = prox(Ht - U) ;  U += H' - Ht
//
// with K, H, U read from global memory once before the loop and H, U and
// the block's iteration count written once after it. The block stops when
//   ||H'-Ht||^2 <= tol*||H'||^2  and  ||H'-H||^2 <= tol*max(||U||^2,||H'||^2)
// (product form: a zero norm never divides), or after max_inner iterations.
//
// Register plan: 256 threads = 4 waves; wave w owns rows 16w..16w+15 of the
// block; lane (q = lane>>4, r = lane&15) owns row r and the columns q + 4j,
// j < J = ceil(F/4), of K, H, U, T and Ht, all in registers. This is at
// once the B-operand layout (k = lane>>4, n = lane&15) and the C/D layout
// (row = lane/16 + 4*reg, col = lane&15) of v_mfma_f64_16x16x4_f64 for the
// TRANSPOSED product Ht^T = Ginv^T * T^T, so the MFMA instances feed the
// registers of one iteration straight into the next with no transpose.
// The VALU instances (runtime rank: every other rank, and the measured
// alternative at 16/32/64) fetch T[r][k] from the lane that owns it with a
// shuffle and read Ginv rows from LDS.
//
// LDS: Ginv zero-padded to 4J x 4J with row stride 4J+1, 16 doubles of
// per-wave partial sums, one stop flag. The four block sums are reduced in
// a fixed order (lane-local over j, xor-shuffles 32..1, then waves 0..3 by
// thread 0): no atomics, so the update is bitwise reproducible.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "launchers.hpp"
#include "mfma_acc.hpp"

namespace {

constexpr int NT = 256;
constexpr int BLOCK_ROWS = 64;

enum : int { NONNEG = 0, L1 = 1, NONNEG_L1 = 2, BOX = 3 };

// th = w / rho for the l1 kinds
__device__ __forceinline__ double prox(double x, int kind, double th,
                                       double lo, double hi) {
  switch (kind) {
    case NONNEG:
      return x < 0.0 ? 0.0 : x;
    case L1: {
      double a = fabs(x) - th;
      a = a < 0.0 ? 0.0 : a;
      return copysign(a, x);
    }
    case NONNEG_L1: {
      const double a = x - th;
      return a < 0.0 ? 0.0 : a;
    }
    default: {
      const double a = x < lo ? lo : x;
      return a > hi ? hi : a;
    }
  }
}

// FC: compile-time rank (0: runtime rank Frt <= 4J). MFMA needs FC == 4J
// and FC % 16 == 0.
template <int FC, int J, bool MFMA>
__global__ void __launch_bounds__(NT)
admm_block_kern(const double * __restrict__ K,
                const double * __restrict__ Ginv,
                const double * __restrict__ rho_p, double * __restrict__ H,
                double * __restrict__ U, int32_t * __restrict__ iters,
                int64_t n, int Frt, int kind, double w, double lo, double hi,
                double inner_tol, int max_inner) {
  constexpr int FP = 4 * J;   // padded rank
  constexpr int LD = FP + 1;  // padded LDS row stride
  static_assert(!MFMA || (FC == FP && FC % 16 == 0), "MFMA needs F = 16k");
  const int F = FC ? FC : Frt;
  extern __shared__ double sm[];  // G[FP*LD] | red[4 waves][4] | flag
  double * Gl = sm;
  double * red = sm + FP * LD;
  int * flag = reinterpret_cast<int *>(red + 16);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wv = tid >> 6;
  const int rl = lane & 15;
  const int q = lane >> 4;
  const int64_t row = (int64_t)blockIdx.x * BLOCK_ROWS + wv * 16 + rl;
  // rows past n are masked, not skipped: they still reach every barrier
  const bool rok = row < n;

  for (int x = tid; x < FP * FP; x += NT) {
    const int k = x / FP, c = x % FP;
    Gl[k * LD + c] = (k < F && c < F) ? Ginv[k * F + c] : 0.0;
  }
  const double rho = *rho_p;
  const double th = w / rho;
  const bool check = inner_tol > 0.0;

  double Kr[J], Hr[J], Ur[J];
  bool ok[J];
  #pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = q + 4 * j;
    ok[j] = rok && (FC || c < F);
    const int64_t off = row * F + c;
    Kr[j] = ok[j] ? K[off] : 0.0;
    Hr[j] = ok[j] ? H[off] : 0.0;
    Ur[j] = ok[j] ? U[off] : 0.0;
  }
  __syncthreads();

  // A operands of the MFMA instances: A[m = lane&15][k = lane>>4] =
  // Ginv[4j + k][16cb + m]. Ranks 16 and 32 keep them in registers for the
  // whole loop; rank 64 (64 doubles a lane) re-reads them from LDS.
  constexpr int NB = FP / 16 > 0 ? FP / 16 : 1;
  constexpr bool GREG = MFMA && FC <= 32;
  double Ga[GREG ? NB : 1][GREG ? J : 1];
  if constexpr (GREG) {
    #pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      #pragma unroll
      for (int j = 0; j < J; ++j)
        Ga[cb][j] = Gl[(4 * j + q) * LD + 16 * cb + rl];
    }
  }

  int it = 0;
  while (it < max_inner) {
    ++it;
    double T[J], Ht[J];
    #pragma unroll
    for (int j = 0; j < J; ++j) T[j] = Kr[j] + rho * (Hr[j] + Ur[j]);

    if constexpr (MFMA) {
      using M = MfmaAcc<double>;
      #pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        M::type acc = M::type{};
        #pragma unroll
        for (int j = 0; j < J; ++j) {
          double a;
          if constexpr (GREG) a = Ga[cb][j];
          else a = Gl[(4 * j + q) * LD + 16 * cb + rl];
          acc = M::mfma(a, T[j], acc);
        }
        // D[m = q + 4i][n = rl] is column 16cb + q + 4i = q + 4*(4cb + i)
        #pragma unroll
        for (int i = 0; i < 4; ++i) Ht[4 * cb + i] = acc[i];
      }
    } else {
      #pragma unroll
      for (int j = 0; j < J; ++j) Ht[j] = 0.0;
      #pragma unroll
      for (int qs = 0; qs < 4; ++qs) {
        #pragma unroll
        for (int js = 0; js < J; ++js) {
          const int k = qs + 4 * js;
          // every lane takes part in the shuffle; k is workgroup-uniform
          const double t = __shfl(T[js], (qs << 4) | rl);
          if (FC || k < F) {
            const double * g = Gl + k * LD + q;
            #pragma unroll
            for (int j = 0; j < J; ++j) Ht[j] += t * g[4 * j];
          }
        }
      }
    }

    double pr = 0.0, pn = 0.0, dr = 0.0, dn = 0.0;
    #pragma unroll
    for (int j = 0; j < J; ++j) {
      double x = prox(Ht[j] - Ur[j], kind, th, lo, hi);
      if (!ok[j]) x = 0.0;
      const double u = (Ur[j] + x) - Ht[j];
      const double a = x - Ht[j];
      const double b = x - Hr[j];
      pr += a * a;
      pn += x * x;
      dr += b * b;
      dn += u * u;
      Hr[j] = x;
      Ur[j] = u;
    }
    if (!check) continue;  // workgroup-uniform

    // Fold the four sums across the wave with 7 shuffles instead of 24:
    // the xor-32 step leaves (pr, pn) in lanes 0..31 and (dr, dn) in lanes
    // 32..63, the xor-16 step one quantity per group of 16 lanes (quantity
    // q in group q), and xor 8..1 finish each group. The order is fixed.
    const bool hi32 = lane & 32, hi16 = lane & 16;
    const double a0 = (hi32 ? dr : pr) + __shfl_xor(hi32 ? pr : dr, 32);
    const double a1 = (hi32 ? dn : pn) + __shfl_xor(hi32 ? pn : dn, 32);
    double b = (hi16 ? a1 : a0) + __shfl_xor(hi16 ? a0 : a1, 16);
    #pragma unroll
    for (int o = 8; o > 0; o >>= 1) b += __shfl_xor(b, o);
    if (rl == 0) red[wv * 4 + q] = b;
    __syncthreads();
    if (tid == 0) {
      double s[4];
      #pragma unroll
      for (int v = 0; v < 4; ++v) {
        s[v] = red[v];
        for (int x = 1; x < NT / WAVE; ++x) s[v] += red[x * 4 + v];
      }
      const double m = s[3] > s[1] ? s[3] : s[1];
      // a NaN fails both comparisons: the block runs to max_inner
      *flag = (s[0] <= inner_tol * s[1] && s[2] <= inner_tol * m) ? 1 : 0;
    }
    __syncthreads();
    // read by every thread before the next barrier: the exit is uniform
    if (*flag) break;
  }

  #pragma unroll
  for (int j = 0; j < J; ++j) {
    if (ok[j]) {
      const int64_t off = row * F + q + 4 * j;
      H[off] = Hr[j];
      U[off] = Ur[j];
    }
  }
  if (tid == 0) iters[blockIdx.x] = it;
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

template <int FC, int J, bool MFMA>
int launch(const double * K, const double * Ginv, const double * rho,
           double * H, double * U, int32_t * iters, int64_t n, int F,
           int kind, double w, double lo, double hi, double inner_tol,
           int max_inner, hipStream_t st) {
  constexpr int FP = 4 * J;
  const size_t lds = ((size_t)FP * (FP + 1) + 16 + 2) * sizeof(double);
  if (int rc = check_lds(lds)) return rc;
  const int64_t nblocks = (n + BLOCK_ROWS - 1) / BLOCK_ROWS;
  hipLaunchKernelGGL((admm_block_kern<FC, J, MFMA>), dim3((uint32_t)nblocks),
                     dim3(NT), lds, st, K, Ginv, rho, H, U, iters, n, F, kind,
                     w, lo, hi, inner_tol, max_inner);
  return launch_rc();
}

}  // namespace

namespace splatt {
namespace hip {

int admm_update(const double * K, const double * Ginv, const double * rho,
                double * H, double * U, int32_t * iters, int64_t n, int F,
                int kind, double w, double lo, double hi, double inner_tol,
                int max_inner, int variant, void * stream) {
  if (n <= 0) return 0;
  const bool spec = F == 16 || F == 32 || F == 64;
  if (F < 1 || F > 64 || kind < 0 || kind > 3 || max_inner < 0
      || variant < 0 || variant > 2 || (variant == 2 && !spec)
      || (n + BLOCK_ROWS - 1) / BLOCK_ROWS > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
#define AARGS K, Ginv, rho, H, U, iters, n, F, kind, w, lo, hi, inner_tol, \
              max_inner, st
  // Ranks 16/32/64 default to the MFMA instances; variant 1 runs them
  // through the generic VALU instance instead (docs/KERNELS.md has both
  // measurements). A compile-time-F VALU instance was tried and dropped:
  // with the rank known the compiler hoists every Ginv read out of the
  // loop and spills at ranks 32 and 64.
  if (spec && variant != 1) {
    if (F == 16) return launch<16, 4, true>(AARGS);
    if (F == 32) return launch<32, 8, true>(AARGS);
    return launch<64, 16, true>(AARGS);
  }
  if (F <= 16) return launch<0, 4, false>(AARGS);
  if (F <= 32) return launch<0, 8, false>(AARGS);
  return launch<0, 16, false>(AARGS);
#undef AARGS
}

}  // namespace hip
}  // namespace splatt
