// Poisson CPD (CP-APR) on gfx950: the fused multiplicative row update.
//
// For output mode m and row i, with Omega_i the nonzeros whose mode-m index
// is i, pi_x the Hadamard product of the other modes' factor rows at x and
// B = A_m diag(lambda), one inner iteration of the row is
//
//   mdl_x  = max(sum_f B[i,f] pi_x[f], eps_div)
//   Phi[i] = sum_{x in Omega_i} (val_x / mdl_x) pi_x
//   v      = max_f |min(B[i,f], 1 - Phi[i,f])|      (KKT violation)
//   stop if inner_tol > 0 and v < inner_tol, else B[i] *= Phi[i]
//
// i.e. a rank reduction at every nonzero feeding an MTTKRP of the ratios in
// the same pass, repeated up to max_inner times. Rows are independent, so
// every row stops on its own violation.
//
// The mode's root-sorted stream makes every Omega_i a contiguous range, cut
// on the host into segments of bounded nnz that never cross a row (the
// planner of the completion kernels). One wave owns one segment. With W the
// power of two >= F, a group of W lanes owns one nonzero at a time, G = 64/W
// nonzeros per wave step, U steps in flight:
//   lane = g * W + c:  group g, column c
//   b      column c of B[i] in a register for the whole segment
//   pi     column c of pi_x: one 8-byte gather per non-root level
//   mdl    b * pi summed over the group by log2 W xor-shuffles
//   acc   += (val / mdl) * pi                       (IEEE division)
// and after the pass the G groups fold over each other by xor-shuffles
// W, 2W, .., 32: every lane then holds column c of the segment's sum.
// The stream is read 64 nonzeros at a time, one line per lane (coalesced),
// and handed to the groups by shuffle, as in ttmc.hip. Columns past F are
// zero through a select with their loads clamped to column 0; the tail of a
// segment has value 0 and the indices of the segment's first nonzero. No
// load is skipped and every lane reaches every shuffle.
//
// A row of one segment (seg_slot < 0) runs the whole inner loop in the wave:
// nothing goes back to memory between iterations, the gathers are repeated,
// and B, Phi, iters, viol0 are stored once. A row of several segments does
// one pass per launch: each wave parks its F partial sums in its slot, and
// apr_fold_kern (one wave per such row) folds the slots in stream order,
// tests the violation and either marks the row done or applies B *= Phi; the
// host relaunches the multi-segment range max_inner times, and a wave whose
// row is done exits at once. No atomics, fixed summation order: bitwise
// reproducible.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "launchers.hpp"

namespace {

constexpr int MAX_RANK = 64;

// non-root levels 1..NO of the stream, BY VALUE in the kernel-arg block
struct AprTab {
  const int32_t * idx[7];
  const double * mats[7];
};

// sum over the W lanes of a group; every lane gets the total
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

// One pass over the segment [s, e): column cc of sum (val / mdl) pi, the
// same in every group.
template <int NO, int W>
__device__ __forceinline__ double
apr_pass(const AprTab & tab, const double * __restrict__ vals, int64_t s,
         int64_t e, int F, int lane, int g, int cc, bool cok, double b,
         double eps_div) {
  constexpr int G = WAVE / W;       // nonzeros per wave step
  constexpr int U = W < 4 ? W : 4;  // steps in flight; divides W
  double acc = 0.0;
  for (int64_t p0 = s; p0 < e; p0 += WAVE) {
    const int64_t q = p0 + lane;
    const bool ok = q < e;
    const int64_t qq = ok ? q : s;
    const double myv = ok ? vals[qq] : 0.0;
    int32_t myi[NO];
    #pragma unroll
    for (int t = 0; t < NO; ++t) myi[t] = tab.idx[t][qq];
    // W steps cover the 64 lines; steps wholly past e are dropped, and U
    // divides W, so a rounded-up count stays inside the 64 lines
    const int nsteps = (int)min64((int64_t)W, (e - p0 + G - 1) / G);
    for (int st = 0; st < nsteps; st += U) {
      double v[U], pi[U];
      #pragma unroll
      for (int u = 0; u < U; ++u) {
        const int src = (st + u) * G + g;
        v[u] = __shfl(myv, src);
        double x = tab.mats[0][(int64_t)__shfl(myi[0], src) * F + cc];
        #pragma unroll
        for (int t = 1; t < NO; ++t)
          x *= tab.mats[t][(int64_t)__shfl(myi[t], src) * F + cc];
        pi[u] = cok ? x : 0.0;
      }
      #pragma unroll
      for (int u = 0; u < U; ++u) {
        const double mdl = fmax(group_sum<W>(b * pi[u]), eps_div);
        acc += (v[u] / mdl) * pi[u];
      }
    }
  }
  // the groups fold over each other in a fixed order
  #pragma unroll
  for (int o = W; o < WAVE; o <<= 1) acc += __shfl_xor(acc, o);
  return acc;
}

template <int NO, int W>
__global__ void __launch_bounds__(WAVE)
apr_seg_kern(const AprTab tab, const double * __restrict__ vals,
             const int64_t * __restrict__ seg_start,
             const int32_t * __restrict__ seg_len,
             const int32_t * __restrict__ seg_row,
             const int32_t * __restrict__ seg_slot, int64_t seg0, int F,
             double eps_div, double inner_tol, int max_inner,
             const int32_t * __restrict__ done, double * __restrict__ ws,
             double * __restrict__ B, double * __restrict__ Phi,
             int32_t * __restrict__ iters, double * __restrict__ viol0) {
  const int lane = threadIdx.x;
  const int c = lane & (W - 1);
  const int g = lane / W;
  const bool cok = c < F;
  const int cc = cok ? c : 0;
  const int64_t sg = seg0 + blockIdx.x;
  const int64_t s = seg_start[sg];
  const int64_t e = s + seg_len[sg];
  const int64_t row = seg_row[sg];
  const int32_t slot = seg_slot[sg];

  if (slot >= 0) {
    // multi-segment row: one pass, the partial goes to the slot
    if (done[row]) return;
    const double b = cok ? B[row * F + cc] : 0.0;
    const double phi =
        apr_pass<NO, W>(tab, vals, s, e, F, lane, g, cc, cok, b, eps_div);
    if (g == 0 && cok) ws[(int64_t)slot * F + c] = phi;
    return;
  }

  // single-segment row: the whole inner loop; v is wave-uniform
  double b = cok ? B[row * F + cc] : 0.0;
  double phi = 0.0, v0 = 0.0;
  int it = 0;
  for (int l = 1; l <= max_inner; ++l) {
    phi = apr_pass<NO, W>(tab, vals, s, e, F, lane, g, cc, cok, b, eps_div);
    const double v =
        group_max<W>(cok ? fabs(fmin(b, 1.0 - phi)) : 0.0);
    it = l;
    if (l == 1) v0 = v;
    if (inner_tol > 0.0 && v < inner_tol) break;
    b *= phi;
  }
  if (g == 0 && cok) {
    B[row * F + c] = b;
    Phi[row * F + c] = phi;
  }
  if (lane == 0) {
    iters[row] = it;
    viol0[row] = v0;
  }
}

// One wave per multi-segment row, lane c = column c: fold the row's slots
// in stream order, then the end of inner iteration `round` for the row.
__global__ void __launch_bounds__(WAVE)
apr_fold_kern(const double * __restrict__ ws,
              const int32_t * __restrict__ mrow,
              const int64_t * __restrict__ mslot, int F, int round,
              double inner_tol, int max_inner, int32_t * __restrict__ done,
              double * __restrict__ B, double * __restrict__ Phi,
              int32_t * __restrict__ iters, double * __restrict__ viol0) {
  const int64_t m = blockIdx.x;
  const int64_t row = mrow[m];
  if (done[row]) return;
  const int c = threadIdx.x;
  const bool cok = c < F;
  const int cc = cok ? c : 0;
  const int64_t a = mslot[m], z = mslot[m + 1];
  double phi = 0.0;
  for (int64_t sl = a; sl < z; ++sl) phi += ws[sl * F + cc];
  const double b = B[row * F + cc];
  const double v = group_max<WAVE>(cok ? fabs(fmin(b, 1.0 - phi)) : 0.0);
  const bool stop = inner_tol > 0.0 && v < inner_tol;
  if (cok) {
    Phi[row * F + c] = phi;
    if (!stop) B[row * F + c] = b * phi;
  }
  if (c == 0) {
    iters[row] = round;
    if (round == 1) viol0[row] = v;
    if (stop || round >= max_inner) done[row] = 1;
  }
}

template <int NO, typename... Args>
int launch_w(int F, dim3 grid, hipStream_t st, Args... args) {
  dim3 block(WAVE);
  // the kernels use no LDS: nothing to check against the device limit
#define APR_W(WW) \
  hipLaunchKernelGGL((apr_seg_kern<NO, WW>), grid, block, 0, st, args...)
  if (F <= 1) APR_W(1);
  else if (F <= 2) APR_W(2);
  else if (F <= 4) APR_W(4);
  else if (F <= 8) APR_W(8);
  else if (F <= 16) APR_W(16);
  else if (F <= 32) APR_W(32);
  else APR_W(64);
#undef APR_W
  return launch_rc();
}

}  // namespace

namespace splatt {
namespace hip {

int apr_segments(const int32_t * const * idx, const double * const * mats,
                 int nother, const double * vals, const int64_t * seg_start,
                 const int32_t * seg_len, const int32_t * seg_row,
                 const int32_t * seg_slot, int64_t seg0, int64_t nseg, int F,
                 double eps_div, double inner_tol, int max_inner,
                 const int32_t * done, double * ws, double * B, double * Phi,
                 int32_t * iters, double * viol0, void * stream) {
  if (nseg <= 0) return 0;
  if (nother < 2 || nother > 7 || F < 1 || F > MAX_RANK || max_inner < 1
      || nseg > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  AprTab tab{};
  for (int t = 0; t < nother; ++t) {
    tab.idx[t] = idx[t];
    tab.mats[t] = mats[t];
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((uint32_t)nseg);
#define LARGS F, grid, st, tab, vals, seg_start, seg_len, seg_row, seg_slot, \
              seg0, F, eps_div, inner_tol, max_inner, done, ws, B, Phi, \
              iters, viol0
  switch (nother) {
    case 2: return launch_w<2>(LARGS);
    case 3: return launch_w<3>(LARGS);
    case 4: return launch_w<4>(LARGS);
    case 5: return launch_w<5>(LARGS);
    case 6: return launch_w<6>(LARGS);
    default: return launch_w<7>(LARGS);
  }
#undef LARGS
}

int apr_fold(const double * ws, const int32_t * mrow, const int64_t * mslot,
             int64_t nm, int F, int round, double inner_tol, int max_inner,
             int32_t * done, double * B, double * Phi, int32_t * iters,
             double * viol0, void * stream) {
  if (nm <= 0) return 0;
  if (F < 1 || F > MAX_RANK || round < 1 || nm > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(apr_fold_kern, dim3((uint32_t)nm), dim3(WAVE), 0,
                     (hipStream_t)stream, ws, mrow, mslot, F, round,
                     inner_tol, max_inner, done, B, Phi, iters, viol0);
  return launch_rc();
}

}  // namespace hip
}  // namespace splatt
