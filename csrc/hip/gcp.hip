// Generalized CPD (GCP) on gfx950: the fused loss-gradient pass.
//
// For a loss l(x, m) summed over the STORED entries of the tensor, output
// mode m and row i, with Omega_i the stored entries whose mode-m index is i
// and pi_x the Hadamard product of the other modes' factor rows at x,
//
//   mdl_x   = sum_f A_m[i,f] pi_x[f]
//   G[i]    = sum_{x in Omega_i} dl/dm(val_x, mdl_x) pi_x
//   frow[i] = sum_{x in Omega_i} l(val_x, mdl_x)             (when wanted)
//
// i.e. a rank reduction at every stored entry feeding an MTTKRP of an
// elementwise function of the result, in one walk of the stream: the
// single-pass sibling of apr.hip, with the same decomposition. The mode's
// root-sorted stream is cut on the host into segments of bounded length that
// never cross a row; one wave owns one segment. With W the power of two
// >= F, a group of W lanes owns one entry at a time, G = 64/W entries per
// wave step, U steps in flight:
//   lane = g * W + c:  group g, column c
//   a      column c of A_m[i] in a register for the whole segment
//   pi     column c of pi_x: one 8-byte gather per non-root level
//   mdl    a * pi summed over the group by log2 W xor-shuffles
//   acc   += dl(val, mdl) * pi
// and after the pass the G groups fold over each other by xor-shuffles
// W, 2W, .., 32. The stream is read 64 entries at a time, one line per lane,
// and handed to the groups by shuffle. No load is skipped and every lane
// reaches every shuffle.
//
// Two rules a general loss needs and apr.hip does not:
//   tails     a step past the end of the segment reads the value 0 and the
//             indices of the segment's first entry, but dl(0, mdl) and
//             l(0, mdl) are not 0: its contribution is dropped by a SELECT on
//             the result (it may be inf or NaN, so not by a multiplication);
//   columns   lanes c >= F have a = pi = 0: they add 0 to mdl, their acc may
//             become NaN and is never stored. The loss value is taken once
//             per ENTRY, by the lane that read the entry's stream line, and
//             summed over the 64 lanes in a fixed xor order.
//
// A row of one segment (seg_slot < 0) stores G[row] (and frow[row]) with
// plain stores. A segment of a longer row parks its F partial sums (F + 1
// with the loss value) in its workspace slot, and gcp_fold_kern (one wave
// per such row) folds the slots in stream order. No atomics, fixed summation
// order: bitwise reproducible. The loss is a wave-uniform runtime switch; the
// loss value is a template flag, so that the gradient-only instances carry
// no logarithm.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "gcp_loss.hpp"
#include "launchers.hpp"

namespace {

constexpr int MAX_RANK = 64;

// non-root levels 1..NO of the stream, BY VALUE in the kernel-arg block
struct GcpTab {
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

// One pass over the segment [s, e): column cc of sum dl(val, mdl) pi in
// `acc`, the same in every group, and sum l(val, mdl) in `facc`, the same
// in every lane.
//
// The derivative is evaluated by every lane of a group at every step. The
// loss VALUE is not: after its reduction a step hands the model value of
// entry j back to lane j (one more shuffle and a select), and once per batch
// of 64 lines every lane evaluates l for its own line, so a logarithm is
// issued once per 64 entries instead of once per G.
template <int NO, int W, bool WANT>
__device__ __forceinline__ void
gcp_pass(const GcpTab & tab, const double * __restrict__ vals, int64_t s,
         int64_t e, int F, int lane, int g, int cc, bool cok, double a,
         int loss, double prm, double & acc_out, double & facc_out) {
  constexpr int G = WAVE / W;       // entries per wave step
  constexpr int U = W < 4 ? W : 4;  // steps in flight; divides W
  double acc = 0.0, facc = 0.0;
  // line `lane` of a batch is reduced at step lane / G by group lane % G
  const int mystep = lane / G;
  const int mysrc = (lane & (G - 1)) * W;
  for (int64_t p0 = s; p0 < e; p0 += WAVE) {
    const int64_t q = p0 + lane;
    const bool ok = q < e;
    const int64_t qq = ok ? q : s;
    const double myv = ok ? vals[qq] : 0.0;
    int32_t myi[NO];
    #pragma unroll
    for (int t = 0; t < NO; ++t) myi[t] = tab.idx[t][qq];
    // lines of this batch that hold an entry of the segment: 1..64
    const int nlive = (int)min64((int64_t)WAVE, e - p0);
    // W steps cover the 64 lines; steps wholly past e are dropped, and U
    // divides W, so a rounded-up count stays inside the 64 lines
    const int nsteps = (nlive + G - 1) / G;
    double mymdl = 0.0;
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
        const double mdl = group_sum<W>(a * pi[u]);
        const double y = loss_deriv(loss, prm, v[u], mdl);
        // a tail step contributes exactly nothing, whatever y is
        const bool live = (st + u) * G + g < nlive;
        acc += live ? y * pi[u] : 0.0;
        if (WANT) {
          const double mj = __shfl(mdl, mysrc);
          mymdl = mystep == st + u ? mj : mymdl;
        }
      }
    }
    if (WANT) {
      // a line past the end contributes exactly nothing, whatever l is
      const double l = loss_value(loss, prm, myv, mymdl);
      facc += ok ? l : 0.0;
    }
  }
  // the groups fold over each other in a fixed order
  #pragma unroll
  for (int o = W; o < WAVE; o <<= 1) acc += __shfl_xor(acc, o);
  acc_out = acc;
  facc_out = WANT ? group_sum<WAVE>(facc) : 0.0;
}

template <int NO, int W, bool WANT>
__global__ void __launch_bounds__(WAVE)
gcp_seg_kern(const GcpTab tab, const double * __restrict__ vals,
             const int64_t * __restrict__ seg_start,
             const int32_t * __restrict__ seg_len,
             const int32_t * __restrict__ seg_row,
             const int32_t * __restrict__ seg_slot, int F, int loss,
             double prm, const double * __restrict__ A,
             double * __restrict__ ws, double * __restrict__ Gout,
             double * __restrict__ frow) {
  const int lane = threadIdx.x;
  const int c = lane & (W - 1);
  const int g = lane / W;
  const bool cok = c < F;
  const int cc = cok ? c : 0;
  const int64_t sg = blockIdx.x;
  const int64_t s = seg_start[sg];
  const int64_t e = s + seg_len[sg];
  const int64_t row = seg_row[sg];
  const int32_t slot = seg_slot[sg];
  const double a = cok ? A[row * F + cc] : 0.0;
  double acc, facc;
  gcp_pass<NO, W, WANT>(tab, vals, s, e, F, lane, g, cc, cok, a, loss, prm,
                        acc, facc);
  if (slot >= 0) {
    // a segment of a multi-segment row: the partials go to the slot
    const int S = F + (WANT ? 1 : 0);
    if (g == 0 && cok) ws[(int64_t)slot * S + c] = acc;
    if (WANT && lane == 0) ws[(int64_t)slot * S + F] = facc;
    return;
  }
  if (g == 0 && cok) Gout[row * F + c] = acc;
  if (WANT && lane == 0) frow[row] = facc;
}

// One wave per multi-segment row, lane c = column c: fold the row's slots
// in stream order. A slot is S = F (+ 1 with frow) doubles.
__global__ void __launch_bounds__(WAVE)
gcp_fold_kern(const double * __restrict__ ws,
              const int32_t * __restrict__ mrow,
              const int64_t * __restrict__ mslot, int F,
              double * __restrict__ Gout, double * __restrict__ frow) {
  const int64_t m = blockIdx.x;
  const int64_t row = mrow[m];
  const int c = threadIdx.x;
  const bool cok = c < F;
  const int cc = cok ? c : 0;
  const int S = F + (frow != nullptr ? 1 : 0);
  const int64_t a = mslot[m], z = mslot[m + 1];
  double acc = 0.0;
  for (int64_t sl = a; sl < z; ++sl) acc += ws[sl * S + cc];
  if (cok) Gout[row * F + c] = acc;
  if (frow != nullptr && c == 0) {
    double f = 0.0;
    for (int64_t sl = a; sl < z; ++sl) f += ws[sl * S + F];
    frow[row] = f;
  }
}

template <int NO, bool WANT, typename... Args>
int launch_w(int F, dim3 grid, hipStream_t st, Args... args) {
  dim3 block(WAVE);
  // the kernels use no LDS: nothing to check against the device limit
#define GCP_W(WW) \
  hipLaunchKernelGGL((gcp_seg_kern<NO, WW, WANT>), grid, block, 0, st, args...)
  if (F <= 1) GCP_W(1);
  else if (F <= 2) GCP_W(2);
  else if (F <= 4) GCP_W(4);
  else if (F <= 8) GCP_W(8);
  else if (F <= 16) GCP_W(16);
  else if (F <= 32) GCP_W(32);
  else GCP_W(64);
#undef GCP_W
  return launch_rc();
}

template <int NO, typename... Args>
int launch_want(bool want, Args... args) {
  return want ? launch_w<NO, true>(args...) : launch_w<NO, false>(args...);
}

}  // namespace

namespace splatt {
namespace hip {

int gcp_segments(const int32_t * const * idx, const double * const * mats,
                 int nother, const double * vals, const int64_t * seg_start,
                 const int32_t * seg_len, const int32_t * seg_row,
                 const int32_t * seg_slot, int64_t nseg, int F, int loss,
                 double param, const double * A, double * ws, double * G,
                 double * frow, void * stream) {
  if (nseg <= 0) return 0;
  if (nother < 2 || nother > 7 || F < 1 || F > MAX_RANK || loss < 0
      || loss >= NLOSS || nseg > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  GcpTab tab{};
  for (int t = 0; t < nother; ++t) {
    tab.idx[t] = idx[t];
    tab.mats[t] = mats[t];
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((uint32_t)nseg);
  const bool want = frow != nullptr;
#define LARGS want, F, grid, st, tab, vals, seg_start, seg_len, seg_row, \
              seg_slot, F, loss, param, A, ws, G, frow
  switch (nother) {
    case 2: return launch_want<2>(LARGS);
    case 3: return launch_want<3>(LARGS);
    case 4: return launch_want<4>(LARGS);
    case 5: return launch_want<5>(LARGS);
    case 6: return launch_want<6>(LARGS);
    default: return launch_want<7>(LARGS);
  }
#undef LARGS
}

int gcp_fold(const double * ws, const int32_t * mrow, const int64_t * mslot,
             int64_t nm, int F, double * G, double * frow, void * stream) {
  if (nm <= 0) return 0;
  if (F < 1 || F > MAX_RANK || nm > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(gcp_fold_kern, dim3((uint32_t)nm), dim3(WAVE), 0,
                     (hipStream_t)stream, ws, mrow, mslot, F, G, frow);
  return launch_rc();
}

}  // namespace hip
}  // namespace splatt
