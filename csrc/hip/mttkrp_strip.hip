// Strip/window flat MTTKRP: root output kept in LDS, one gather served
// from L2.
//
// The unstaged v7 kernel (mttkrp_flat.hip) misses L2 on every factor-row
// gather when the factors are far larger than the 4 MiB per-XCD L2: two
// 128-B lines per nonzero at rank 16 f64 and 3 modes. Bucketing the stream
// by a gathered mode's row range makes that mode's rows L2-resident, but
// with output in global memory every (output row, bucket) run costs an
// atomic, and L2-sized buckets shred the runs. Here the output rows of a
// workgroup live in LDS for the whole walk, so the bucket count costs
// nothing in global memory:
//
//   strip   a contiguous range of at most tile_rows output rows and the
//           stream range [p0, p1) of their nonzeros (planned on the host,
//           csrc/core/partition.cpp plan_strips; nnz-balanced, a row heavier
//           than the cap is split between strips and flagged as shared);
//   window  inside a strip the nonzeros are sorted by idx_w / window_rows of
//           one gathered level w (splatt_amd/csf.py), so at any moment the
//           workgroups of a launch gather level w from one or two windows of
//           its factor that fit the L2.
//
// One workgroup owns one strip: it zeroes a tile of tile_rows x F doubles
// (row stride padded by 16 B), walks the strip's stream once in stored
// order and stores the tile to `out` — plain coalesced stores, except the
// rows it shares with a neighbouring strip, which are added atomically into
// the pre-zeroed `out`. Per nonzero the work is v7's: a column group of F
// lanes stages a 32-nonzero window of every stream with one non-temporal
// load per 128-B line, redistributes it with __shfl, gathers in batches of
// 8 (the window level, idx[0] / mats[0], with plain loads; the other levels,
// whose rows miss anyway, non-temporally, so that they are the first lines
// the L2 gives up) and folds consecutive nonzeros of one output row in a
// register; on a
// row change the partial goes to the tile with an LDS f64 add. The groups
// of a workgroup take the strip's windows round-robin, so the workgroup
// advances through the buckets together (2048 nonzeros per round at rank
// 16).
//
// One launch per dispatch: the grid is min(wgs, nstrips) workgroups, and
// workgroup b takes the strips b, b + grid, b + 2 grid, ... (the passes). A
// strip's windows are cut into `ngroups` groups (bounds[s][g] ..
// bounds[s][g + 1]); the tile is zeroed once, the groups are walked in order
// and the tile is stored once. Workgroups left alone drift apart by far more
// than the time one of them spends in a window (profiles/
// amazon_strip_window.md), so they would not share a window; after each
// group every workgroup therefore passes pace(), a counter barrier over the
// grid, which keeps the workgroups of a pass within one group of windows.
//
// pace() carries no data: a strip's tile and unshared rows belong to one
// workgroup and shared rows are added atomically, so a workgroup that stops
// waiting loses L2 hits and nothing else. That is what bounds every wait.
// One lane adds 1 to the arrival counter (relaxed, agent scope) and polls it
// with relaxed loads and s_sleep until it reaches ticket x grid or the
// wall-clock budget runs out; on expiry it counts a time-out and the
// workgroup stops waiting for the rest of the launch, but goes on arriving,
// so that the others' targets stay reachable. A grid that is not co-resident
// therefore costs one budget per workgroup, never a hang. Every workgroup
// makes exactly passes x ngroups calls, also one with no strip in the last
// pass. Without a pace buffer there are no waits: one unpaced launch.
//
// Run-ahead. A full barrier pays the slowest of the grid at every group, and
// the pacing needs less: only that the workgroups stay within a bounded
// stretch of the window factor. With a slots buffer (a ring of S = 8
// counters, one 128-B line each) a workgroup's call number t (0-based,
// continuous over groups and passes) adds 1 to slot t % S and, for t >= R,
// waits until slot (t - R) % S has reached grid x ((t - R) / S + 1), i.e.
// until every workgroup has arrived at ticket t - R: it may lead the slowest
// by R groups (R + 1 while the slowest has not arrived), R = `ahead` in
// 0..S-1, and R = 0 is the barrier again. The ring is sound because
// S >= R + 1: a workgroup arrives at ticket t + S only after it has seen
// ticket t + S - 1 - R >= t complete, so until every workgroup has arrived
// at t, slot t % S counts arrivals at tickets t, t - S, t - 2S, ... only and
// reaches the target exactly when the last one arrives. A timed-out
// workgroup no longer waits but goes on arriving, possibly early at a later
// ticket of a slot's class: that can only end other waits sooner, and no
// result depends on a wait. The arrival total (word 0) is then added once
// per workgroup at the end of the kernel, not once per call. Lane 0 also
// sums its waits and counts the calls in which it had to poll (words 65 and
// 66 of the pace buffer, and, with a trace buffer, four words per workgroup:
// XCC id, wait sum, polled calls, longest wait).
#include <hip/hip_runtime.h>
#include <cstdint>

#include <type_traits>

#include "device_common.hpp"
#include "launchers.hpp"

namespace {

constexpr int STRIP_THREADS = 1024;   // 16 waves: 4 per SIMD, one block/CU
constexpr int STRIP_PAD = 2;          // doubles added to the tile row stride

template <typename T, int N>
__device__ __forceinline__ void ldnt_vec(const T * p, T (&r)[N]) {
  if constexpr (N == 1) {
    r[0] = ldnt(p);
  } else {
    using VT = T __attribute__((ext_vector_type(N)));
    const VT v = __builtin_nontemporal_load(reinterpret_cast<const VT *>(p));
    #pragma unroll
    for (int i = 0; i < N; ++i) r[i] = v[i];
  }
}

// the strip descriptors (device arrays of nstrips entries) and the streams
struct StripArgs {
  const int32_t * key, * i0, * i1, * i2;
  const double * m0, * m1, * m2;
  const int32_t * row0, * nrows, * flags;
  const int64_t * bounds;      // [nstrips][ngroups + 1] stream positions
  int ngroups;
  int64_t nnz;                 // length of the streams
  uint32_t * pace;             // PACE_* words, zeroed per launch; or null
  int64_t budget;              // longest wait, in wall_clock64() ticks
  uint32_t * slots;            // ring of PACE_SLOTS counters, zeroed per
                               // launch; or null: wait on PACE_ARRIVALS
  int ahead;                   // run-ahead R, 0 .. PACE_SLOTS - 1
  uint32_t * trace;            // [grid][4] per-workgroup words; or null
};

// words of the pace buffer, each on a 128-B line of its own
constexpr int PACE_ARRIVALS = 0;      // pace() calls, all workgroups
constexpr int PACE_TIMEOUTS = 32;     // workgroups that stopped waiting
constexpr int PACE_LONGEST = 64;      // longest wait, wall_clock64() ticks
// two more words of that line, written once per workgroup and launch
constexpr int PACE_WAITSUM = 65;      // sum of all waits, ticks (mod 2^32)
constexpr int PACE_POLLED = 66;       // pace() calls that had to poll
constexpr int PACE_WORDS = 96;
// the slot ring of the run-ahead protocol, each slot on a line of its own
constexpr int PACE_SLOTS = 8;
constexpr int SLOT_STRIDE = 32;
constexpr int SLOT_WORDS = PACE_SLOTS * SLOT_STRIDE;

template <int F, int NOTHER, typename VS>
__global__ void __launch_bounds__(STRIP_THREADS)
mttkrp_strip_kern(const StripArgs a, const VS * __restrict__ vals,
                  int64_t nstrips, int tile_rows,
                  double * __restrict__ out) {
  constexpr int R = WAVE / F;
  constexpr int W = 32;                          // stream window (nnz)
  constexpr int EPL = (F >= W) ? 1 : W / F;      // int32 elements per lane
  constexpr int VPL = (sizeof(VS) == 8 && EPL > 1) ? EPL / 2 : EPL;
  constexpr int NVL = EPL / VPL;                 // vals loads per window
  constexpr int CH = W / NVL;                    // elements per vals load
  constexpr int GB = 8;                          // gather sub-batch
  constexpr int LD = F + STRIP_PAD;              // tile row stride
  extern __shared__ double tile[];

  const int32_t * __restrict__ key = a.key;
  const int32_t * __restrict__ i0 = a.i0;
  const int32_t * __restrict__ i1 = a.i1;
  const int32_t * __restrict__ i2 = a.i2;
  const double * __restrict__ m0 = a.m0;
  const double * __restrict__ m1 = a.m1;
  const double * __restrict__ m2 = a.m2;

  // the grid barrier after a group of windows; state of the polling lane
  // ticket and waiting in registers; lane 0's statistics (longest wait, sum
  // of waits, both in ticks and saturating, and polled calls) in LDS, since
  // only the wait path touches them
  uint32_t ticket = 0;           // pace() calls made so far
  bool waiting = true;
  __shared__ uint32_t pstat[3];
  if (threadIdx.x == 0) pstat[0] = pstat[1] = pstat[2] = 0;
  auto pace = [&]() {
    if (!a.pace) return;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t t = ticket++;
      // the counter arrived at, and the one waited on with its target
      uint32_t * arrive = a.pace + PACE_ARRIVALS;
      uint32_t * watch = arrive;
      uint32_t target = ticket * gridDim.x;
      bool wait = waiting;
      if (a.slots) {
        const uint32_t R = (uint32_t)a.ahead;
        arrive = a.slots + (t % PACE_SLOTS) * SLOT_STRIDE;
        wait = waiting && t >= R;
        if (wait) {
          const uint32_t u = t - R;
          watch = a.slots + (u % PACE_SLOTS) * SLOT_STRIDE;
          target = (u / PACE_SLOTS + 1) * gridDim.x;
        }
      }
      __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      if (wait) {
        const int64_t t0 = (int64_t)wall_clock64();
        bool spun = false;
        while (__hip_atomic_load(watch, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) < target) {
          spun = true;
          if ((int64_t)wall_clock64() - t0 >= a.budget) {
            atomicAdd(a.pace + PACE_TIMEOUTS, 1u);
            waiting = false;     // sticky: no more waits in this launch
            break;
          }
          __builtin_amdgcn_s_sleep(8);
        }
        const int64_t dt64 = (int64_t)wall_clock64() - t0;
        const uint32_t dt =
            (uint32_t)(dt64 < 0xFFFFFFFFll ? dt64 : 0xFFFFFFFFll);
        if (dt > pstat[0]) pstat[0] = dt;
        if (spun) {
          pstat[1] = pstat[1] + dt < dt ? 0xFFFFFFFFu : pstat[1] + dt;
          ++pstat[2];
        }
      }
    }
    __syncthreads();
  };

  const int lane = threadIdx.x & (WAVE - 1);
  const int c = lane % F;
  const int g = lane / F;
  const int gbase = g * F;
  const int slot = c & (W / EPL - 1);            // F=64: lanes 32.. mirror
  const int nlg = (blockDim.x / WAVE) * R;      // lane groups
  const int gid = (threadIdx.x / WAVE) * R + g;

  for (int64_t s = blockIdx.x; s - blockIdx.x < nstrips; s += gridDim.x) {
    if (s >= nstrips) {          // no strip in the last pass: keep the count
      for (int grp = 0; grp < a.ngroups; ++grp) pace();
      break;
    }
    const int32_t row0 = a.row0[s];
    const int nr = a.nrows[s] < tile_rows ? a.nrows[s] : tile_rows;
    const int fl = a.flags[s];
    const int64_t * bnd = a.bounds + s * (a.ngroups + 1);

    for (int e = threadIdx.x; e < nr * LD; e += blockDim.x) tile[e] = 0.0;
    __syncthreads();

    int32_t cur = -1;
    double acc = 0.0;
    // a row outside the strip (a stream that does not match its descriptors)
    // is dropped, never written past the tile
    auto flush = [&]() {
      const uint32_t lr = (uint32_t)(cur - row0);
      if (lr < (uint32_t)nr) unsafeAtomicAdd(&tile[lr * LD + c], acc);
    };
    auto fold = [&](int32_t k, double x) {
      if (k != cur) {
        flush();
        acc = 0.0;
        cur = k;
      }
      acc += x;
    };
    // one element at a time, every lane of the group reading the same words
    // (the last line of the stream only)
    auto scalar = [&](int64_t pa, int64_t pb) {
      for (int64_t p = pa; p < pb; ++p) {
        double x = (double)ldnt(&vals[p]) * m0[(int64_t)ldnt(&i0[p]) * F + c]
                   * ldnt(&m1[(int64_t)ldnt(&i1[p]) * F + c]);
        if constexpr (NOTHER > 2)
          x *= ldnt(&m2[(int64_t)ldnt(&i2[p]) * F + c]);
        fold(ldnt(&key[p]), x);
      }
    };

    for (int grp = 0; grp < a.ngroups; ++grp) {
      const int64_t p0 = bnd[grp], p1 = bnd[grp + 1];
      // windows are the 128-B lines of the streams (all 128-B aligned): the
      // lines that overlap [p0, p1) go round-robin over the lane groups. A
      // line cut by p0 or p1 is staged and gathered whole (its other
      // elements belong to a neighbouring group or strip, so their indices
      // are valid rows) and only its elements inside the range are folded:
      // one lane group walking them one by one would hold every workgroup
      // of the launch at the next pace(). A lane's open run (cur, acc)
      // carries over into the next group.
      const int64_t wlo = p0 / W;
      const int64_t wend = p1 > p0 ? (p1 + W - 1) / W : wlo;
      // the stream's last line, if it is not a whole one, is not staged
      const int64_t whi = min64(wend, a.nnz / W);

      for (int64_t w = wlo + gid; w < whi; w += nlg) {
        const int64_t pw = w * W;
        // elements [lo, hi) of the line are the group's
        const int lo = pw < p0 ? (int)(p0 - pw) : 0;
        const int hi = pw + W > p1 ? (int)(p1 - pw) : W;
        const int64_t ps = pw + slot * EPL;
        int32_t kreg[EPL], i0reg[EPL], i1reg[EPL], i2reg[EPL];
        VS vreg[NVL][VPL];
        ldnt_vec(key + ps, kreg);
        ldnt_vec(i0 + ps, i0reg);
        ldnt_vec(i1 + ps, i1reg);
        if constexpr (NOTHER > 2) ldnt_vec(i2 + ps, i2reg);
        #pragma unroll
        for (int k = 0; k < NVL; ++k)
          ldnt_vec(vals + pw + k * CH + slot * VPL, vreg[k]);
        #pragma unroll
        for (int k = 0; k < NVL; ++k) {
          #pragma unroll 1
          for (int h = 0; h < CH; h += GB) {
            const int ub = k * CH + h;
            double vv[GB], a0[GB], a1[GB], a2[GB];
            #pragma unroll
            for (int u = 0; u < GB; ++u) {
              const int src = gbase + ub / EPL + u / EPL;
              vv[u] = (double)__shfl(vreg[k][u % VPL],
                                     gbase + h / VPL + u / VPL, WAVE);
              const int32_t j0 = __shfl(i0reg[u % EPL], src, WAVE);
              const int32_t j1 = __shfl(i1reg[u % EPL], src, WAVE);
              a0[u] = m0[(int64_t)j0 * F + c];
              a1[u] = ldnt(&m1[(int64_t)j1 * F + c]);
              if constexpr (NOTHER > 2) {
                const int32_t j2 = __shfl(i2reg[u % EPL], src, WAVE);
                a2[u] = ldnt(&m2[(int64_t)j2 * F + c]);
              }
            }
            #pragma unroll
            for (int u = 0; u < GB; ++u) {
              double x = vv[u] * a0[u] * a1[u];
              if constexpr (NOTHER > 2) x *= a2[u];
              const int32_t k = __shfl(kreg[u % EPL],
                                       gbase + ub / EPL + u / EPL, WAVE);
              if (ub + u >= lo && ub + u < hi) fold(k, x);
            }
          }
        }
      }

      if (wend > whi && gid == nlg - 1)
        scalar(whi * W > p0 ? whi * W : p0, p1);
      if (grp + 1 < a.ngroups) pace();
    }
    flush();
    __syncthreads();

    for (int e = threadIdx.x; e < nr * F; e += blockDim.x) {
      const int lr = e / F, cc = e % F;
      const double v = tile[lr * LD + cc];
      double * o = &out[(int64_t)(row0 + lr) * F + cc];
      if ((lr == 0 && (fl & 1)) || (lr == nr - 1 && (fl & 2)))
        atomic_add_g(o, v);
      else
        *o = v;                // the strip's other rows are this workgroup's
    }
    // the stores of the fast workgroups overlap the walk of the slow ones
    if (a.pace) pace(); else __syncthreads();
  }
  if (a.pace && threadIdx.x == 0) {
    const uint32_t lw = pstat[0], ws = pstat[1], polled = pstat[2];
    if (lw > 0) atomicMax(a.pace + PACE_LONGEST, lw);
    if (polled > 0) {
      atomicAdd(a.pace + PACE_WAITSUM, ws);
      atomicAdd(a.pace + PACE_POLLED, polled);
    }
    // with the ring nobody waits on the total: one add per workgroup
    if (a.slots) atomicAdd(a.pace + PACE_ARRIVALS, ticket);
    if (a.trace) {
      // HW_REG_XCC_ID, bits 3:0: the XCD this workgroup ran on
      const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11));
      uint32_t * tr = a.trace + (size_t)blockIdx.x * 4;
      tr[0] = xcc;
      tr[1] = ws;
      tr[2] = polled;
      tr[3] = lw;
    }
  }
}

// largest dynamic LDS request a block may make on the current device
inline int lds_limit() {
  static int limit = -1;
  if (limit < 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock,
                                 dev) != hipSuccess)
      return 0;
    limit = v;
  }
  return limit;
}

inline int cu_count() {
  static int n = -1;
  if (n < 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount,
                                 dev) != hipSuccess)
      return 0;
    n = v;
  }
  return n;
}

// wall_clock64() ticks per millisecond (the constant-rate clock of pace())
inline int wall_khz() {
  static int khz = -1;
  if (khz < 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, dev)
               != hipSuccess || v <= 0)
      return 0;
    khz = v;
  }
  return khz;
}

struct StripLaunch {
  StripArgs a;
  const void * vals;
  int64_t nstrips;
  int wgs;
  int tile_rows;
  double * out;
  hipStream_t st;
};

// One kernel instance: raise its dynamic-LDS limit to `lds` bytes (once per
// size), then either answer the resident-workgroup count (L == nullptr) or
// clear the pace words and launch the grid.
template <int F, int NOTHER, typename VS>
int strip_inst(const StripLaunch * L, int lds, int * wgs) {
  static int lds_set = 0;
  auto kern = mttkrp_strip_kern<F, NOTHER, VS>;
  if (lds > lds_set) {
    const hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void *>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    lds_set = lds;
  }
  if (!L) {
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, kern, STRIP_THREADS, (size_t)lds);
    if (e != hipSuccess) return (int)e;
    *wgs = per_cu * cu_count();
    return wall_khz() > 0 ? 0 : (int)hipErrorInvalidDevice;
  }
  if (L->a.pace) {
    // a memset node under capture: a replay starts from zero as well
    const hipError_t e = hipMemsetAsync(
        L->a.pace, 0, PACE_WORDS * sizeof(uint32_t), L->st);
    if (e != hipSuccess) return (int)e;
  }
  if (L->a.slots) {
    const hipError_t e = hipMemsetAsync(
        L->a.slots, 0, SLOT_WORDS * sizeof(uint32_t), L->st);
    if (e != hipSuccess) return (int)e;
  }
  const int64_t n = L->nstrips < L->wgs ? L->nstrips : L->wgs;
  hipLaunchKernelGGL(kern, dim3((uint32_t)n), dim3(STRIP_THREADS),
                     (size_t)lds, L->st, L->a,
                     static_cast<const VS *>(L->vals), L->nstrips,
                     L->tile_rows, L->out);
  return launch_rc();
}

template <typename VS>
int strip_dispatch(const StripLaunch * L, int tile_rows, int rank, int nother,
                   int * wgs) {
  if (!(rank == 16 || rank == 32 || rank == 64) || nother < 2 || nother > 3
      || tile_rows < 1)
    return -1;
  const int64_t lds = (int64_t)tile_rows * (rank + STRIP_PAD) * 8;
  if (lds > lds_limit()) return -2;
#define SI(F_, N_) return strip_inst<F_, N_, VS>(L, (int)lds, wgs)
#define SF(N_) \
  switch (rank) { case 16: SI(16, N_); case 32: SI(32, N_); \
                  default: SI(64, N_); }
  if (nother == 2) { SF(2); }
  SF(3);
#undef SF
#undef SI
}

}  // namespace

namespace splatt {
namespace hip {

int strip_wgs(int rank, int nother, bool vals32, int tile_rows) {
  int wgs = 0;
  const int rc = vals32
      ? strip_dispatch<float>(nullptr, tile_rows, rank, nother, &wgs)
      : strip_dispatch<double>(nullptr, tile_rows, rank, nother, &wgs);
  return rc == 0 ? wgs : 0;
}

template <typename VS>
int mttkrp_strip(const int32_t * key, const int32_t * const * idx,
                 const double * const * mats, const VS * vals,
                 const int32_t * s_row0, const int32_t * s_nrows,
                 const int32_t * s_flags, const int64_t * s_bounds,
                 int ngroups, int64_t nstrips, int tile_rows, int wgs,
                 int64_t nnz, double * out, int rank, int nother,
                 void * stream, uint32_t * pace, int pace_us,
                 uint32_t * slots, int ahead, uint32_t * trace) {
  if (nstrips <= 0) return 0;
  if (wgs < 1 || ngroups < 1 || nother < 2 || nother > 3 || pace_us < 0)
    return -1;
  if (ahead < 0 || ahead >= PACE_SLOTS || (ahead > 0 && !slots)
      || ((slots || trace) && !pace))
    return -1;
  // windows are the streams' 128-B lines
  uintptr_t bits = (uintptr_t)key | (uintptr_t)vals;
  for (int t = 0; t < nother; ++t) bits |= (uintptr_t)idx[t];
  if (bits & 127) return -1;
  StripLaunch L{{key, idx[0], idx[1], nother > 2 ? idx[2] : nullptr, mats[0],
                 mats[1], nother > 2 ? mats[2] : nullptr, s_row0, s_nrows,
                 s_flags, s_bounds, ngroups, nnz, pace,
                 (int64_t)pace_us * wall_khz() / 1000, slots, ahead, trace},
                vals, nstrips, wgs, tile_rows, out, (hipStream_t)stream};
  return strip_dispatch<VS>(&L, tile_rows, rank, nother, nullptr);
}

#define STRIP_SIG(VS)                                                      \
  const int32_t *, const int32_t * const *, const double * const *,        \
  const VS *, const int32_t *, const int32_t *, const int32_t *,           \
  const int64_t *, int, int64_t, int, int, int64_t, double *, int, int,    \
  void *, uint32_t *, int, uint32_t *, int, uint32_t *
template int mttkrp_strip<double>(STRIP_SIG(double));
template int mttkrp_strip<float>(STRIP_SIG(float));
#undef STRIP_SIG

int strip_wall_khz() { return wall_khz(); }

}  // namespace hip
}  // namespace splatt
