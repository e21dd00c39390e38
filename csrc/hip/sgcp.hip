// Stochastic generalized CPD (Kolda & Hong 2020) on gfx950: the fused
// sampled-gradient pass and the fused Adam step.
//
// A sample is n = p + q coordinates, UNSORTED and different at every step:
// p draws of stored entries (value x_j) followed by q draws of cells (value
// 0). With mdl_j the model value at sample j, the semi-stratified estimator
// of the gradient of sum over ALL cells of l(x, mdl) is
//
//   y_j  = wnz * (dl(x_j, mdl_j) - dl(0, mdl_j))     j <  p
//   y_j  = wz  *  dl(0, mdl_j)                        j >= p
//   G_t[i_t(j)] += y_j * prod_{u != t} A_u[i_u(j)]    for every mode t
//
// and the loss estimate is the same with l in place of dl, summed.
//
// sgcp_grad_kern is sample-parallel. With W the power of two >= F, a group
// of W lanes owns one sample, G = 64/W samples per wave step, U steps in
// flight; the waves of the grid stride over the sample:
//   lane = g * W + c:  group g, column c
//   a[t]   column c of A_t[i_t(j)]: one 8-byte gather per mode, the row a
//          coalesced F*8-byte line. All U*NM gathers of a lane are issued
//          before the first is used: the rows are random, so the pass is
//          bound by latency before bandwidth, and U*NM = 10..16 loads per
//          lane at 4-8 waves per SIMD is what keeps the memory system busy
//   mdl    prod_t a[t] summed over the group by log2 W xor-shuffles
//   pi_t   the leave-one-out product from prefix and suffix products in
//          registers (never a division: factor entries may be 0)
//   G_t   += y * pi_t by the native f64 global atomic add, NM per lane
// The stored/cell boundary p may fall inside a wave step: the kind of a
// sample is j < p per group. A wave whose samples are all cell draws (a
// wave-uniform test) skips dl(x, .) and l(x, .).
//
// Three rules, as in gcp.hip:
//   tails     a group past the end of the sample reads sample 0; it is
//             dropped by a PREDICATE on its atomics and its loss term, not
//             by a multiplication: dl(0, mdl) may be inf or NaN;
//   columns   lanes c >= F load nothing, add 0 to mdl and issue no atomics;
//   shuffles  every lane reaches every shuffle.
//
// With WANT the loss term of a sample is taken once, by lane c == 0 of its
// group, summed over the wave in a fixed xor order and stored as ONE double
// per wave in `partials` (the caller adds them up): no atomic on a scalar,
// and the loss estimate is bitwise reproducible. The gradients are NOT:
// the order in which atomics to one row arrive varies from run to run, as
// for the default MTTKRP.
//
// adam_step_kern is one grid-stride elementwise pass over the flat parameter
// buffer: reads x, g, m, v, writes x, m, v and g = 0. Contraction is off, so
// every product and sum rounds once, as in the torch formula.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "gcp_loss.hpp"
#include "launchers.hpp"

namespace {

constexpr int MAX_RANK = 64;
constexpr int BLOCK = 256;               // 4 waves
constexpr int WAVES = BLOCK / WAVE;
constexpr int MAX_BLOCKS = 2048;         // 256 CUs x 8 resident blocks

// the factors and their gradients, BY VALUE in the kernel-arg block
struct SgcpTab {
  const double * mats[8];
  double * grads[8];
};

// sum over the W lanes of a group; every lane gets the total
template <int W>
__device__ __forceinline__ double group_sum(double x) {
  #pragma unroll
  for (int o = W >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// steps in flight: U * NM gathers per lane, 10..16
template <int NM> constexpr int steps_in_flight() { return NM <= 4 ? 4 : 2; }

template <int NM, int W, bool WANT>
__global__ void __launch_bounds__(BLOCK)
sgcp_grad_kern(const SgcpTab tab, const int32_t * __restrict__ inds,
               const double * __restrict__ vals, int64_t n, int64_t p, int F,
               int loss, double prm, double wnz, double wz,
               double * __restrict__ partials) {
  constexpr int G = WAVE / W;
  constexpr int U = steps_in_flight<NM>();
  constexpr int PER = G * U;             // samples per wave iteration
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = lane & (W - 1);
  const int g = lane / W;
  const bool cok = c < F;
  const int64_t wid = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
  const int64_t nw = (int64_t)gridDim.x * WAVES;
  double facc = 0.0;
  for (int64_t j0 = wid * PER; j0 < n; j0 += nw * PER) {
    int32_t row[U][NM];
    double x[U], a[U][NM];
    bool live[U];
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + u * G + g;
      live[u] = j < n;
      const int64_t jj = live[u] ? j : 0;
      x[u] = vals[jj];
      #pragma unroll
      for (int t = 0; t < NM; ++t) row[u][t] = inds[t * n + jj];
    }
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      #pragma unroll
      for (int t = 0; t < NM; ++t) {
        a[u][t] = 0.0;
        if (cok) a[u][t] = tab.mats[t][(int64_t)row[u][t] * F + c];
      }
    }
    // wave-uniform: samples are ordered, stored draws first
    const bool any_stored = j0 < p;
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      // suf[t] = prod_{s > t} a[s]
      double suf[NM];
      suf[NM - 1] = 1.0;
      #pragma unroll
      for (int t = NM - 2; t >= 0; --t) suf[t] = suf[t + 1] * a[u][t + 1];
      const double mdl = group_sum<W>(a[u][0] * suf[0]);
      const bool stored = j0 + u * G + g < p;
      const double d0 = loss_deriv(loss, prm, 0.0, mdl);
      double y = wz * d0;
      if (any_stored) {
        const double dx = loss_deriv(loss, prm, x[u], mdl);
        y = stored ? wnz * (dx - d0) : y;
      }
      if (WANT) {
        const double l0 = loss_value(loss, prm, 0.0, mdl);
        double l = wz * l0;
        if (any_stored) {
          const double lx = loss_value(loss, prm, x[u], mdl);
          l = stored ? wnz * (lx - l0) : l;
        }
        // a tail group contributes exactly nothing, whatever l is
        facc += (live[u] && c == 0) ? l : 0.0;
      }
      const bool add = live[u] && cok;
      double pre = 1.0;
      #pragma unroll
      for (int t = 0; t < NM; ++t) {
        if (add)
          atomic_add_g(tab.grads[t] + ((int64_t)row[u][t] * F + c),
                       y * (pre * suf[t]));
        pre *= a[u][t];
      }
    }
  }
  if (WANT) {
    facc = group_sum<WAVE>(facc);
    if (lane == 0) partials[wid] = facc;
  }
}

int64_t grid_blocks(int64_t n, int W, int NM) {
  const int U = NM <= 4 ? 4 : 2;
  const int64_t per_block = (int64_t)(WAVE / W) * U * WAVES;
  const int64_t b = (n + per_block - 1) / per_block;
  return b < MAX_BLOCKS ? b : MAX_BLOCKS;
}

int width_of(int F) {
  int W = 1;
  while (W < F) W <<= 1;
  return W;
}

template <int NM, bool WANT, typename... Args>
int launch_w(int W, dim3 grid, hipStream_t st, Args... args) {
  dim3 block(BLOCK);
  // the kernel uses no LDS: nothing to check against the device limit
#define SGCP_W(WW) \
  case WW: \
    hipLaunchKernelGGL((sgcp_grad_kern<NM, WW, WANT>), grid, block, 0, st, \
                       args...); \
    break
  switch (W) {
    SGCP_W(1); SGCP_W(2); SGCP_W(4); SGCP_W(8); SGCP_W(16); SGCP_W(32);
    default: SGCP_W(64);
  }
#undef SGCP_W
  return launch_rc();
}

template <int NM, typename... Args>
int launch_want(bool want, Args... args) {
  return want ? launch_w<NM, true>(args...) : launch_w<NM, false>(args...);
}

__global__ void __launch_bounds__(BLOCK)
adam_step_kern(double * __restrict__ x, double * __restrict__ g,
               double * __restrict__ m, double * __restrict__ v, int64_t n,
               double lr, double beta1, double omb1, double beta2,
               double omb2, double eps, double c1, double c2, bool bounded,
               double lower) {
  #pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += stride) {
    const double gi = g[i];
    const double mi = beta1 * m[i] + omb1 * gi;
    const double vi = beta2 * v[i] + (omb2 * gi) * gi;
    double xi = x[i] - (lr * (mi * c1)) / (sqrt(vi * c2) + eps);
    // a NaN stays a NaN, as with torch's clamp
    if (bounded) xi = xi < lower ? lower : xi;
    m[i] = mi;
    v[i] = vi;
    x[i] = xi;
    g[i] = 0.0;
  }
}

}  // namespace

namespace splatt {
namespace hip {

int64_t sgcp_nparts(int64_t n, int nmodes, int F) {
  if (n <= 0 || F < 1 || F > MAX_RANK) return 0;
  return grid_blocks(n, width_of(F), nmodes) * WAVES;
}

int sgcp_grad(const int32_t * inds, const double * vals, int64_t n, int64_t p,
              const double * const * mats, double * const * grads, int nmodes,
              int F, int loss, double param, double wnz, double wz,
              double * partials, void * stream) {
  if (nmodes < 3 || nmodes > 8 || F < 1 || F > MAX_RANK || loss < 0
      || loss >= NLOSS || n < 1 || p < 0 || p > n)
    return (int)hipErrorInvalidValue;
  SgcpTab tab{};
  for (int t = 0; t < nmodes; ++t) {
    tab.mats[t] = mats[t];
    tab.grads[t] = grads[t];
  }
  hipStream_t st = (hipStream_t)stream;
  const int W = width_of(F);
  dim3 grid((uint32_t)grid_blocks(n, W, nmodes));
  const bool want = partials != nullptr;
#define LARGS want, W, grid, st, tab, inds, vals, n, p, F, loss, param, wnz, \
              wz, partials
  switch (nmodes) {
    case 3: return launch_want<3>(LARGS);
    case 4: return launch_want<4>(LARGS);
    case 5: return launch_want<5>(LARGS);
    case 6: return launch_want<6>(LARGS);
    case 7: return launch_want<7>(LARGS);
    default: return launch_want<8>(LARGS);
  }
#undef LARGS
}

int adam_step(double * x, double * g, double * m, double * v, int64_t n,
              double lr, double beta1, double beta2, double eps, double c1,
              double c2, bool bounded, double lower, void * stream) {
  if (n <= 0) return 0;
  int64_t blocks = (n + BLOCK - 1) / BLOCK;
  if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
  hipLaunchKernelGGL(adam_step_kern, dim3((uint32_t)blocks), dim3(BLOCK), 0,
                     (hipStream_t)stream, x, g, m, v, n, lr, beta1,
                     1.0 - beta1, beta2, 1.0 - beta2, eps, c1, c2, bounded,
                     lower);
  return launch_rc();
}

}  // namespace hip
}  // namespace splatt
