// TTMc (tensor-times-matrix chain) on gfx950: the hot kernel of the sparse
// Tucker decomposition (HOOI).
//
// For output mode n and row i, with Omega_i the nonzeros whose mode-n index
// is i,
//
//   Y[i, :] = sum_{x in Omega_i} val_x * KRON_{t != n} U_t[i_t(x), :]
//
// The mode's root-sorted stream makes every Omega_i a contiguous range, cut
// on the host into segments of bounded nnz that never cross a row (the
// planner of the completion kernels). Per row this is a GEMM A^T B whose K
// dimension is the nonzeros of the row:
//   A[x][a] = val_x * U_l1[i_l1(x), a]                 (level 1, RA columns)
//   B[x][b] = prod_{l >= 2} U_l[i_l(x), b_l]           (levels 2.., PB columns,
//             b = mixed-radix (b_2, .., b_last), last level fastest)
// and Y[i] is the RA x PB matrix A^T B, stored row-major: the output is in
// CSF LEVEL order, [rows][R_l1][R_l2]..[R_last].
//
// One wave owns one segment and TBC consecutive 16-column tiles of B
// (blockIdx.y picks the chunk of tiles; a wide PB re-walks the segment once
// per chunk). Four nonzeros k = lane>>4 feed one v_mfma_f64_16x16x4_f64 per
// (A tile, B tile):
//   A operand [m = lane&15][k] = val * U_l1[.., 16*ta + m]
//   B operand [k][n = lane&15] = B[.., 16*tb + n]
//   D tile (ta, tb): row lane/16 + 4*reg, column lane&15  (MfmaAcc<double>)
// The stream is read 64 nonzeros at a time, one line per lane (coalesced),
// and handed to the groups of four by shuffle: fetching it per group would
// spend a whole-wave load on four distinct addresses, and measured 2x the
// call time at the NELL-2 shape.
// Columns past RA / PB are zero-filled through a select and the K tail of
// a segment through a zero value; their loads are clamped to column 0 /
// the segment's first nonzero, never skipped and never out of range.
//
// A row that fits one segment is stored straight to `out`. A row that spans
// several segments parks each partial in a workspace slot of P doubles (the
// layout of an output row); ttmc_reduce_kern folds the slots in stream
// order. No atomics, fixed summation order: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "device_common.hpp"
#include "launchers.hpp"
#include "mfma_acc.hpp"

namespace {

constexpr int MAX_RANK = 32;
constexpr int MAX_COLS = 4096;

// non-root levels 1..NO of the stream, BY VALUE in the kernel-arg block
struct TtmcTab {
  const int32_t * idx[7];
  const double * mats[7];
  int rank[7];
};

template <int NO, int TA, int TBC>
__global__ void __launch_bounds__(WAVE)
ttmc_mfma_kern(const TtmcTab tab, const double * __restrict__ vals,
               const int64_t * __restrict__ seg_start,
               const int32_t * __restrict__ seg_len,
               const int32_t * __restrict__ seg_row,
               const int32_t * __restrict__ seg_slot,
               int64_t seg0, int64_t slot0, int PB,
               double * __restrict__ ws, double * __restrict__ out) {
  constexpr int NBL = NO - 1;           // levels of the B group
  constexpr int U = TBC >= 4 ? 2 : 4;   // groups of four nonzeros in flight
  using M = MfmaAcc<double>;
  using Acc = M::type;

  const int lane = threadIdx.x;
  const int c = lane & 15;
  const int k = lane >> 4;
  const int64_t sg = seg0 + blockIdx.x;
  const int64_t s = seg_start[sg];
  const int64_t e = s + seg_len[sg];
  const int RA = tab.rank[0];
  const int tb0 = blockIdx.y * TBC;

  // this lane's operand columns, clamped to column 0 where masked
  int ca[TA];
  bool aok[TA];
  #pragma unroll
  for (int ta = 0; ta < TA; ++ta) {
    const int a = 16 * ta + c;
    aok[ta] = a < RA;
    ca[ta] = aok[ta] ? a : 0;
  }
  int cb[TBC][NBL];
  bool bok[TBC];
  #pragma unroll
  for (int j = 0; j < TBC; ++j) {
    const int b = 16 * (tb0 + j) + c;
    bok[j] = b < PB;
    int rem = bok[j] ? b : 0;
    #pragma unroll
    for (int t = NBL - 1; t >= 0; --t) {
      const int R = tab.rank[t + 1];
      cb[j][t] = rem % R;
      rem /= R;
    }
  }

  Acc acc[TA][TBC];
  #pragma unroll
  for (int ta = 0; ta < TA; ++ta) {
    #pragma unroll
    for (int j = 0; j < TBC; ++j) acc[ta][j] = Acc{};
  }

  // 64 nonzeros per block: lane l fetches the stream line of nonzero
  // p0 + l (one coalesced load per column), then every group of four
  // takes its lines by shuffle. Past the segment's end the value is 0 and
  // the indices are those of the segment's first nonzero.
  for (int64_t p0 = s; p0 < e; p0 += WAVE) {
    const int64_t q = p0 + lane;
    const bool ok = q < e;
    const int64_t qq = ok ? q : s;
    const double myv = ok ? vals[qq] : 0.0;
    int32_t myi[NO];
    #pragma unroll
    for (int t = 0; t < NO; ++t) myi[t] = tab.idx[t][qq];
    const int ngroups = (int)min((int64_t)(WAVE / 4), (e - p0 + 3) / 4);
    for (int g0 = 0; g0 < ngroups; g0 += U) {
      double av[U][TA];
      double bv[U][TBC];
      #pragma unroll
      for (int u = 0; u < U; ++u) {
        const int src = ((g0 + u) * 4 + k) & (WAVE - 1);
        const double v = __shfl(myv, src);
        const int64_t ra = (int64_t)__shfl(myi[0], src) * RA;
        #pragma unroll
        for (int ta = 0; ta < TA; ++ta) {
          const double x = v * tab.mats[0][ra + ca[ta]];
          av[u][ta] = aok[ta] ? x : 0.0;
        }
        int64_t rb[NBL];
        #pragma unroll
        for (int t = 0; t < NBL; ++t)
          rb[t] = (int64_t)__shfl(myi[t + 1], src) * tab.rank[t + 1];
        #pragma unroll
        for (int j = 0; j < TBC; ++j) {
          double x = tab.mats[1][rb[0] + cb[j][0]];
          #pragma unroll
          for (int t = 1; t < NBL; ++t)
            x *= tab.mats[t + 1][rb[t] + cb[j][t]];
          bv[u][j] = bok[j] ? x : 0.0;
        }
      }
      #pragma unroll
      for (int u = 0; u < U; ++u) {
        #pragma unroll
        for (int ta = 0; ta < TA; ++ta) {
          #pragma unroll
          for (int j = 0; j < TBC; ++j)
            acc[ta][j] = M::mfma(av[u][ta], bv[u][j], acc[ta][j]);
        }
      }
    }
  }

  // single-segment row: straight to the output row; otherwise to the slot
  const int64_t P = (int64_t)RA * PB;
  const int32_t slot = seg_slot[sg];
  double * base = slot >= 0 ? ws + ((int64_t)slot - slot0) * P
                            : out + (int64_t)seg_row[sg] * P;
  #pragma unroll
  for (int ta = 0; ta < TA; ++ta) {
    #pragma unroll
    for (int j = 0; j < TBC; ++j) {
      const int b = 16 * (tb0 + j) + c;
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = 16 * ta + M::crow(lane, i);
        if (a < RA && b < PB) base[(int64_t)a * PB + b] = acc[ta][j][i];
      }
    }
  }
}

// One workgroup per (multi-segment row, 256 output columns): fold the row's
// slots in stream order.
__global__ void __launch_bounds__(256)
ttmc_reduce_kern(const double * __restrict__ ws,
                 const int32_t * __restrict__ mrow,
                 const int64_t * __restrict__ mslot, int64_t m0,
                 int64_t slot0, int P, double * __restrict__ out) {
  const int64_t m = m0 + blockIdx.x;
  const int64_t a = mslot[m] - slot0;
  const int64_t b = mslot[m + 1] - slot0;
  const int el = blockIdx.y * 256 + threadIdx.x;
  if (el >= P) return;
  double sum = 0.0;
  for (int64_t sl = a; sl < b; ++sl) sum += ws[sl * P + el];
  out[(int64_t)mrow[m] * P + el] = sum;
}

template <int NO, int TA>
int launch_tb(const TtmcTab & tab, const double * vals,
              const int64_t * seg_start, const int32_t * seg_len,
              const int32_t * seg_row, const int32_t * seg_slot, int64_t seg0,
              int64_t nseg, int64_t slot0, int PB, double * ws, double * out,
              hipStream_t st) {
  const int TB = (PB + 15) / 16;
  const int tbc = TB >= 3 ? 4 : TB;
  dim3 grid((uint32_t)nseg, (uint32_t)((TB + tbc - 1) / tbc)), block(WAVE);
#define TARGS tab, vals, seg_start, seg_len, seg_row, seg_slot, seg0, slot0, \
              PB, ws, out
  // the kernels use no LDS: nothing to check against the device limit
  switch (tbc) {
    case 1: hipLaunchKernelGGL((ttmc_mfma_kern<NO, TA, 1>), grid, block, 0, st, TARGS); break;
    case 2: hipLaunchKernelGGL((ttmc_mfma_kern<NO, TA, 2>), grid, block, 0, st, TARGS); break;
    default: hipLaunchKernelGGL((ttmc_mfma_kern<NO, TA, 4>), grid, block, 0, st, TARGS); break;
  }
#undef TARGS
  return launch_rc();
}

template <int NO, typename... Args>
int launch_ta(int RA, Args... args) {
  return RA <= 16 ? launch_tb<NO, 1>(args...) : launch_tb<NO, 2>(args...);
}

}  // namespace

namespace splatt {
namespace hip {

int ttmc_max_cols() { return MAX_COLS; }

int ttmc_segments(const int32_t * const * idx, const double * const * mats,
                  const int * ranks, int nother, const double * vals,
                  const int64_t * seg_start, const int32_t * seg_len,
                  const int32_t * seg_row, const int32_t * seg_slot,
                  int64_t seg0, int64_t nseg, int64_t slot0, double * ws,
                  double * out, void * stream) {
  if (nseg <= 0) return 0;
  if (nother < 2 || nother > 7 || nseg > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  TtmcTab tab{};
  int64_t PB = 1;
  for (int t = 0; t < nother; ++t) {
    if (ranks[t] < 1 || ranks[t] > MAX_RANK) return (int)hipErrorInvalidValue;
    tab.idx[t] = idx[t];
    tab.mats[t] = mats[t];
    tab.rank[t] = ranks[t];
    if (t > 0) PB *= ranks[t];
    if (PB * ranks[0] > MAX_COLS) return (int)hipErrorInvalidValue;
  }
  hipStream_t st = (hipStream_t)stream;
#define LARGS ranks[0], tab, vals, seg_start, seg_len, seg_row, seg_slot, \
              seg0, nseg, slot0, (int)PB, ws, out, st
  switch (nother) {
    case 2: return launch_ta<2>(LARGS);
    case 3: return launch_ta<3>(LARGS);
    case 4: return launch_ta<4>(LARGS);
    case 5: return launch_ta<5>(LARGS);
    case 6: return launch_ta<6>(LARGS);
    default: return launch_ta<7>(LARGS);
  }
#undef LARGS
}

int ttmc_reduce(const double * ws, const int32_t * mrow,
                const int64_t * mslot, int64_t m0, int64_t nm, int64_t slot0,
                int P, double * out, void * stream) {
  if (nm <= 0) return 0;
  if (P < 1 || P > MAX_COLS || nm > 0x7FFFFFFF)
    return (int)hipErrorInvalidValue;
  dim3 grid((uint32_t)nm, (uint32_t)((P + 255) / 256)), block(256);
  hipLaunchKernelGGL(ttmc_reduce_kern, grid, block, 0, (hipStream_t)stream,
                     ws, mrow, mslot, m0, slot0, P, out);
  return launch_rc();
}

}  // namespace hip
}  // namespace splatt
