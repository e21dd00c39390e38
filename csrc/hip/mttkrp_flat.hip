// CDNA4 flat ("expanded-CSF") MTTKRP — the default device hot path.
//
// Motivation (measured, profiles/): the hierarchical CSF walk is a serial
// dependent-load chain per fiber; on power-law tensors with short fibers it
// runs latency-bound at ~1.5% of HBM roofline. This kernel linearizes the
// computation: for every nonzero p (in CSF-sorted order)
//     prod[p] = vals[p] * PROD_t mats[t][ idx_t[p] ]     (t = non-out modes)
//     out[key[p], :] += prod[p]
// where idx_t / key are the per-nnz ancestor-label expansions of the CSF
// levels (splatt_amd/csf.py ancestor_expand). Because nonzeros are sorted,
// `key` is piecewise-constant, so each 64/F-lane column group walks a
// contiguous sub-span serially, folds products into a register accumulator,
// and emits one hardware f64/f32 atomic-add per key RUN — not per nonzero.
// The factor-row gathers of a batch are independent, so the loop is
// throughput-bound, not latency-bound (the CSF-walk family in
// mttkrp_kernels.hip is kept as a comparison algorithm, reference-style
// `splatt bench -a`).
//
// Capability parity: same operator as reference mttkrp.c:390-1278 at any
// output depth, any nmodes in {3,4,5}, f32/f64, any rank (spec F in
// {4,8,16,32,64}, generic otherwise).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>

#include <type_traits>

#include "device_common.hpp"
#include "launchers.hpp"
#include "store_types.hpp"

namespace {
using splatt_store::bf16;
using splatt_store::to_compute;

// ------------------------------------------------- staged spec kernel (v2)
// F lanes per column group, R = 64/F groups each walking a contiguous
// sub-span. Having every lane of a group load the same stream words
// (key/idx/vals) caps memory-level parallelism by the VGPR cost of the
// unroll (the retired v1, docs/KERNELS.md). v2 stages streams COALESCED —
// lane slot c of a group loads element pb+c of each stream in one
// instruction per F nonzeros — and redistributes them with ds_bpermute
// (__shfl); the factor-row gathers then issue in independent batches of 8,
// giving ~4x the outstanding gathers per wave at lower VGPR pressure.
template <typename V, int F, int NOTHER, typename S = V>
__global__ void __launch_bounds__(256)
mttkrp_flat2_kern(const int32_t * __restrict__ key,
                  const int32_t * __restrict__ i0,
                  const int32_t * __restrict__ i1,
                  const int32_t * __restrict__ i2,
                  const int32_t * __restrict__ i3,
                  const S * __restrict__ m0, const S * __restrict__ m1,
                  const S * __restrict__ m2, const S * __restrict__ m3,
                  const V * __restrict__ vals, int64_t nnz, int64_t span,
                  V * __restrict__ out) {
  constexpr int R = WAVE / F;
  constexpr int GB = (F >= 8) ? 8 : F;       // gather sub-batch
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x / WAVE)
                      + (threadIdx.x / WAVE);
  const int c = lane % F;
  const int g = lane / F;
  const int gbase = g * F;
  int64_t p0, p1;
  if (!group_range(wid, g, R, nnz, span, p0, p1)) return;

  int32_t cur = key[p0];
  V acc = (V)0;
  for (int64_t pb = p0; pb < p1; pb += F) {
    const int nb = (int)min64((int64_t)F, p1 - pb);       // group-uniform
    const int64_t ps = pb + (c < nb ? c : nb - 1);        // clamped slot
    const int32_t kreg = ldnt(&key[ps]);
    const int32_t i0reg = ldnt(&i0[ps]);
    const int32_t i1reg = ldnt(&i1[ps]);
    const int32_t i2reg = (NOTHER > 2) ? ldnt(&i2[ps]) : 0;
    const int32_t i3reg = (NOTHER > 3) ? ldnt(&i3[ps]) : 0;
    const V vreg = ldnt(&vals[ps]);
    for (int ub = 0; ub < nb; ub += GB) {
      const int ne = nb - ub < GB ? nb - ub : GB;         // group-uniform
      int32_t kk[GB];
      V vv[GB];
      S a0[GB], a1[GB], a2[GB], a3[GB];
      #pragma unroll
      for (int u = 0; u < GB; ++u) {
        const int src = gbase + (u < ne ? ub + u : ub);
        kk[u] = __shfl(kreg, src, WAVE);
        vv[u] = __shfl(vreg, src, WAVE);
        const int32_t j0 = __shfl(i0reg, src, WAVE);
        const int32_t j1 = __shfl(i1reg, src, WAVE);
        a0[u] = m0[(int64_t)j0 * F + c];
        a1[u] = m1[(int64_t)j1 * F + c];
        if (NOTHER > 2) {
          const int32_t j2 = __shfl(i2reg, src, WAVE);
          a2[u] = m2[(int64_t)j2 * F + c];
        }
        if (NOTHER > 3) {
          const int32_t j3 = __shfl(i3reg, src, WAVE);
          a3[u] = m3[(int64_t)j3 * F + c];
        }
      }
      #pragma unroll
      for (int u = 0; u < GB; ++u) {
        if (u >= ne) break;
        V x = vv[u] * to_compute(a0[u], (V)0) * to_compute(a1[u], (V)0);
        if (NOTHER > 2) x *= to_compute(a2[u], (V)0);
        if (NOTHER > 3) x *= to_compute(a3[u], (V)0);
        if (kk[u] != cur) {
          atomic_add_g(&out[(int64_t)cur * F + c], acc);
          acc = (V)0;
          cur = kk[u];
        }
        acc += x;
      }
    }
  }
  atomic_add_g(&out[(int64_t)cur * F + c], acc);
}

// --------------------------------- full-line staged spec kernel (v7)
// v2's F-element stream window is 64 B of an int32 stream at F=16 (32 B at
// F=8): two (four) consecutive windows touch the same 128-B line, the
// loads are non-temporal and a batch of random row gathers sits between
// them, so the line is fetched from HBM again on every touch
// (profiles/amazon_stream_lines.md). v7 stages a fixed window of W=32
// nonzeros whatever F is, so every stream load instruction of a column
// group covers whole 128-B lines and every line is loaded by exactly one
// instruction:
//   int32 streams  lane slot s loads EPL = 32/F consecutive elements
//                  (4/8/16-B load); element e of the window lives in lane
//                  gbase + e/EPL, component e%EPL
//   vals (f64)     NVL = 2 loads of 128 B each for F <= 16 (element e:
//                  load e/CH, lane gbase + (e%CH)/VPL, component e%VPL);
//                  f32 vals follow the int32 layout
// The value STREAM type VS is separate from the compute type V: VS = float
// with V = double reads a 4-byte copy of values that are all f32-exact
// (splatt_amd/mttkrp.py narrows once per CSF) with the int32 layout, one
// load per window, and widens each value once after the shuffle.
// Windows are aligned to 32 elements of the underlying allocation: the
// launcher passes `phase` (elements from the preceding 128-B boundary to
// the first element) and rounds span so sub-spans start on window
// boundaries; the partial windows at the two ends of a launch take a
// scalar per-element path. Gather batch (8) and the fold order within a
// sub-span are those of v2.
//
// RP = true replaces the key stream by row pointers (root output of a
// key-sorted stream): a sub-span binary-searches its first row once, keeps
// the position `next` at which the row ends and, one boundary ahead,
// `next2`; when the walk reaches `next` it flushes, advances (skipping
// empty rows, which therefore get no atomic) and loads the boundary after
// the new `next` — a load nothing waits on before the following run change.
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

template <typename V, int F, int NOTHER, typename S, bool RP, typename VS = V>
__global__ void __launch_bounds__(256)
mttkrp_flat7_kern(const int32_t * __restrict__ key,
                  const int64_t * __restrict__ rowptr, int64_t nrows,
                  int64_t goff,
                  const int32_t * __restrict__ i0,
                  const int32_t * __restrict__ i1,
                  const int32_t * __restrict__ i2,
                  const int32_t * __restrict__ i3,
                  const S * __restrict__ m0, const S * __restrict__ m1,
                  const S * __restrict__ m2, const S * __restrict__ m3,
                  const VS * __restrict__ vals, int64_t nnz, int64_t span,
                  int phase, V * __restrict__ out) {
  constexpr int R = WAVE / F;
  constexpr int W = 32;                          // stream window (nnz)
  constexpr int EPL = (F >= W) ? 1 : W / F;      // int32 elements per lane
  constexpr int VPL = (sizeof(VS) == 8 && EPL > 1) ? EPL / 2 : EPL;
  constexpr int NVL = EPL / VPL;                 // vals loads per window
  constexpr int CH = W / NVL;                    // elements per vals load
  constexpr int GB = 8;                          // gather sub-batch
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x / WAVE)
                      + (threadIdx.x / WAVE);
  const int c = lane % F;
  const int g = lane / F;
  const int gbase = g * F;
  const int slot = c & (W / EPL - 1);            // F=64: lanes 32.. mirror
  // positions q are relative to the 128-B-aligned base `phase` elements
  // before the first nonzero; the launch covers [phase, phase + nnz)
  const int64_t gs = span / R;                   // multiple of W
  const int64_t q0 = wid * span + g * gs;
  const int64_t a = q0 > phase ? q0 : (int64_t)phase;
  const int64_t b = min64(q0 + gs, phase + nnz);
  if (a >= b) return;

  int32_t cur;
  int64_t next = 0, next2 = 0;
  int nrel = 0;             // `next` relative to the window, clamped to W
  int64_t pwg = 0;          // global stream position of the window start
  if constexpr (RP) {
    const int64_t P = a - phase + goff;
    int64_t l = 0, h = nrows;          // rowptr[l] <= P < rowptr[h]
    while (h - l > 1) {
      const int64_t mid = (l + h) >> 1;
      if (rowptr[mid] <= P) l = mid; else h = mid;
    }
    cur = (int32_t)l;
    next = rowptr[l + 1];
    next2 = rowptr[min64(l + 2, nrows)];
  } else {
    cur = key[a - phase];
  }
  V acc = (V)0;

  auto fold = [&](int e, int32_t k, V x) {
    if constexpr (RP) {
      if (e >= nrel) {
        atomic_add_g(&out[(int64_t)cur * F + c], acc);
        acc = (V)0;
        const int64_t P = pwg + e;
        do {                           // skips rows with no nonzeros
          ++cur;
          next = next2;
          next2 = rowptr[min64((int64_t)cur + 2, nrows)];
        } while (P >= next && (int64_t)cur + 1 < nrows);
        nrel = (int)min64(next - pwg, (int64_t)W);
      }
    } else {
      if (k != cur) {
        atomic_add_g(&out[(int64_t)cur * F + c], acc);
        acc = (V)0;
        cur = k;
      }
    }
    acc += x;
  };

  for (int64_t qb = a & ~(int64_t)(W - 1); qb < b; qb += W) {
    const int64_t pw = qb - phase;     // stream index of window element 0
    if constexpr (RP) {
      pwg = pw + goff;
      nrel = (int)min64(next - pwg, (int64_t)W);
    }
    if (qb >= a && qb + W <= b) {
      const int64_t ps = pw + slot * EPL;
      int32_t kreg[EPL], i0reg[EPL], i1reg[EPL], i2reg[EPL], i3reg[EPL];
      VS vreg[NVL][VPL];
      if constexpr (!RP) ldnt_vec(key + ps, kreg);
      ldnt_vec(i0 + ps, i0reg);
      ldnt_vec(i1 + ps, i1reg);
      if constexpr (NOTHER > 2) ldnt_vec(i2 + ps, i2reg);
      if constexpr (NOTHER > 3) ldnt_vec(i3 + ps, i3reg);
      #pragma unroll
      for (int k = 0; k < NVL; ++k)
        ldnt_vec(vals + pw + k * CH + slot * VPL, vreg[k]);
      // batches of one vals chunk stay a rolled loop (the unrolled form
      // hoists the next batch's gathers and costs a wave of occupancy);
      // GB is a multiple of EPL and VPL, so register components stay
      // compile-time and only the source lane depends on the batch
      #pragma unroll
      for (int k = 0; k < NVL; ++k) {
        #pragma unroll 1
        for (int h = 0; h < CH; h += GB) {
          const int ub = k * CH + h;
          V vv[GB];
          S a0[GB], a1[GB], a2[GB], a3[GB];
          #pragma unroll
          for (int u = 0; u < GB; ++u) {
            const int src = gbase + ub / EPL + u / EPL;
            vv[u] = (V)__shfl(vreg[k][u % VPL], gbase + h / VPL + u / VPL,
                              WAVE);
            const int32_t j0 = __shfl(i0reg[u % EPL], src, WAVE);
            const int32_t j1 = __shfl(i1reg[u % EPL], src, WAVE);
            a0[u] = m0[(int64_t)j0 * F + c];
            a1[u] = m1[(int64_t)j1 * F + c];
            if constexpr (NOTHER > 2) {
              const int32_t j2 = __shfl(i2reg[u % EPL], src, WAVE);
              a2[u] = m2[(int64_t)j2 * F + c];
            }
            if constexpr (NOTHER > 3) {
              const int32_t j3 = __shfl(i3reg[u % EPL], src, WAVE);
              a3[u] = m3[(int64_t)j3 * F + c];
            }
          }
          #pragma unroll
          for (int u = 0; u < GB; ++u) {
            V x = vv[u] * to_compute(a0[u], (V)0) * to_compute(a1[u], (V)0);
            if constexpr (NOTHER > 2) x *= to_compute(a2[u], (V)0);
            if constexpr (NOTHER > 3) x *= to_compute(a3[u], (V)0);
            // the key is redistributed at the fold, not with the batch:
            // kreg is live anyway and the batch needs 8 registers less
            int32_t k = 0;
            if constexpr (!RP)
              k = __shfl(kreg[u % EPL], gbase + ub / EPL + u / EPL, WAVE);
            fold(ub + u, k, x);
          }
        }
      }
    } else {
      // partial window at an end of the launch: one element at a time,
      // every lane of the group reading the same stream words
      const int e0 = (int)((a > qb ? a : qb) - qb);
      const int e1 = (int)(min64(b, qb + W) - qb);
      for (int e = e0; e < e1; ++e) {
        const int64_t p = pw + e;
        V x = (V)ldnt(&vals[p])
              * to_compute(m0[(int64_t)ldnt(&i0[p]) * F + c], (V)0)
              * to_compute(m1[(int64_t)ldnt(&i1[p]) * F + c], (V)0);
        if constexpr (NOTHER > 2)
          x *= to_compute(m2[(int64_t)ldnt(&i2[p]) * F + c], (V)0);
        if constexpr (NOTHER > 3)
          x *= to_compute(m3[(int64_t)ldnt(&i3[p]) * F + c], (V)0);
        int32_t k = 0;
        if constexpr (!RP) k = ldnt(&key[p]);
        fold(e, k, x);
      }
    }
  }
  atomic_add_g(&out[(int64_t)cur * F + c], acc);
}

// A/B lever: SPLATT_MTTKRP_U=1 makes v7 decline, so that v2 runs in its
// place (the same-binary oracle of the tests). Any other value is as unset.
inline bool force_v2() {
  const char * e = getenv("SPLATT_MTTKRP_U");
  return e && atoi(e) == 1;
}

// Elements between the preceding 128-B line boundary of the int32 streams
// and their first element, or -1 when the streams of this launch are not
// co-aligned (some stream's line boundaries fall on other elements).
template <typename VS>
inline int stream_phase(const int32_t * key, const int32_t * const idx[8],
                        int nother, const VS * vals) {
  const int phase = (int)(((uintptr_t)idx[0] >> 2) & 31);
  if (key && (int)(((uintptr_t)key >> 2) & 31) != phase) return -1;
  for (int t = 1; t < nother; ++t)
    if ((int)(((uintptr_t)idx[t] >> 2) & 31) != phase) return -1;
  if ((uintptr_t)vals % sizeof(VS)) return -1;
  if ((int)(((uintptr_t)vals / sizeof(VS)) & 31) != phase) return -1;
  return phase;
}

// v7 launcher; rowptr != nullptr selects the row-pointer variant (key may
// then be null). Returns false, launching nothing, when v7 does not apply:
// rank outside 8/16/32/64, more than 4 other modes, SPLATT_MTTKRP_U=1,
// streams that are not co-aligned, or the one instance that would lose
// occupancy (below).
// span is pick_span() rounded DOWN to a multiple of 32*R (R = 64/F groups
// per wave: 256/128/64/32 at F = 8/16/32/64) so that every group's sub-span
// is a whole number of 32-element windows. The 256 minimum and the 16384
// clamp are multiples of all four, so both survive the rounding.
template <typename V, typename S, typename VS = V>
bool launch_flat7(const int32_t * key, const int64_t * rowptr, int64_t nrows,
                  int64_t goff, const int32_t * const idx[8],
                  const S * const mats[8], const VS * vals, int64_t nnz,
                  V * out, int rank, int nother, hipStream_t st) {
  if (!(rank == 8 || rank == 16 || rank == 32 || rank == 64)) return false;
  if (nother < 2 || nother > 4 || force_v2()) return false;
  // the one instance whose 16-B staging costs occupancy: rank 8, 3 modes,
  // f64 values and factors needs 102 (row pointers) / 106 (key) VGPRs
  // against v2's 95, i.e. 4 waves/SIMD instead of 5, and forcing 5 spills
  // to scratch. It stays on v2. (With an f32 value stream the staging is
  // 4 B a lane narrower: 88 / 92 VGPRs, 5 waves/SIMD, so that one runs.)
  if (rank == 8 && nother == 2 && sizeof(VS) == 8 && sizeof(S) == 8)
    return false;
  const int phase = stream_phase<VS>(key, idx, nother, vals);
  if (phase < 0) return false;
  const int64_t quantum = 32 * (WAVE / rank);
  const int64_t span = pick_span(nnz) / quantum * quantum;
  const int64_t nwaves = (phase + nnz + span - 1) / span;
  const int wpb = 4;
  const int64_t nblocks = (nwaves + wpb - 1) / wpb;
  dim3 grid((uint32_t)nblocks), block(wpb * WAVE);
#define ARGS7 key, rowptr, nrows, goff, idx[0], idx[1], idx[2], idx[3], \
              mats[0], mats[1], mats[2], mats[3], vals, nnz, span, phase, out
#define L7(F_, N_) \
  if (rowptr) \
    hipLaunchKernelGGL((mttkrp_flat7_kern<V, F_, N_, S, true, VS>), grid, \
                       block, 0, st, ARGS7); \
  else \
    hipLaunchKernelGGL((mttkrp_flat7_kern<V, F_, N_, S, false, VS>), grid, \
                       block, 0, st, ARGS7)
#define L7F(N_) \
  switch (rank) { case 8: L7(8, N_); break; case 16: L7(16, N_); break; \
                  case 32: L7(32, N_); break; default: L7(64, N_); break; }
  switch (nother) {
    case 2: L7F(2); break;
    case 3: L7F(3); break;
    default: L7F(4); break;
  }
#undef L7F
#undef L7
#undef ARGS7
  return true;
}

// ------------------------------------------------------ generic-rank kernel
// lane = column (chunked by 64), wave walks its span serially. Correctness
// path for ranks outside the spec set.
// up to 7 other modes (8-mode tensors, reference SPLATT_MAX_NMODES);
// idx/mats arrive BY VALUE in the kernel-arg struct (no device-side table,
// no upload: the launch stays async and hipGraph-capturable)
template <typename V>
struct PtrTab {
  const int32_t * idx[8];
  const V * mats[8];
};

template <typename V, int NOTHER>
__global__ void __launch_bounds__(256)
mttkrp_flat_generic_kern(const int32_t * __restrict__ key,
                         const PtrTab<V> tab,
                         const V * __restrict__ vals, int64_t nnz,
                         int64_t span, int rank, V * __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wid = (int64_t)blockIdx.x * (blockDim.x / WAVE)
                      + (threadIdx.x / WAVE);
  const int64_t p0 = wid * span;
  if (p0 >= nnz) return;
  const int64_t p1 = min64(nnz, p0 + span);
  const int32_t * ip[NOTHER];
  const V * mp[NOTHER];
  #pragma unroll
  for (int t = 0; t < NOTHER; ++t) { ip[t] = tab.idx[t]; mp[t] = tab.mats[t]; }
  for (int cb = 0; cb < rank; cb += WAVE) {
    const int c = cb + lane;
    if (c >= rank) break;
    int32_t cur = key[p0];
    V acc = (V)0;
    for (int64_t p = p0; p < p1; ++p) {
      V x = vals[p];
      #pragma unroll
      for (int t = 0; t < NOTHER; ++t)
        x *= mp[t][(int64_t)ip[t][p] * rank + c];
      const int32_t k = key[p];
      if (k != cur) {
        atomic_add_g(&out[(int64_t)cur * rank + c], acc);
        acc = (V)0;
        cur = k;
      }
      acc += x;
    }
    atomic_add_g(&out[(int64_t)cur * rank + c], acc);
  }
}

// what v7 declines on a key stream: v2 at spec ranks and <= 5 modes, the
// generic kernel otherwise. The generic kernel reads factors of the compute
// type only: with a reduced-precision store (S != V) outside v2's shapes
// this returns false, launching nothing.
template <typename V, typename S>
bool launch_flat(const int32_t * key, const int32_t * const idx[8],
                 const S * const mats[8], const V * vals, int64_t nnz,
                 V * out, int rank, int nother, hipStream_t st) {
  const int64_t span = pick_span(nnz);
  const int64_t nwaves = (nnz + span - 1) / span;
  const int wpb = 4;
  const int64_t nblocks = (nwaves + wpb - 1) / wpb;
  dim3 grid((uint32_t)nblocks), block(wpb * WAVE);

#define ARGS key, idx[0], idx[1], idx[2], idx[3], mats[0], mats[1], mats[2], \
             mats[3], vals, nnz, span, out
#define L2(F_, N_) \
  hipLaunchKernelGGL((mttkrp_flat2_kern<V, F_, N_, S>), grid, block, 0, st, ARGS)
#define LF(N_) \
  switch (rank) { case 4: L2(4, N_); break; case 8: L2(8, N_); break; \
                  case 16: L2(16, N_); break; case 32: L2(32, N_); break; \
                  default: L2(64, N_); break; }
  if (spec_ok(rank) && nother <= 4) {
    switch (nother) {
      case 2: LF(2); break;
      case 3: LF(3); break;
      default: LF(4); break;
    }
    return true;
  }
#undef LF
#undef L2
#undef ARGS
  if constexpr (std::is_same<S, V>::value) {
    // generic path (odd ranks or >5 modes): pointer tables travel by value
    // in the kernel-arg block — async launch, graph-capturable, no cleanup
    PtrTab<V> tab{};
    for (int t = 0; t < nother; ++t) { tab.idx[t] = idx[t]; tab.mats[t] = mats[t]; }
#define GARGS key, tab, vals, nnz, span, rank, out
    switch (nother) {
      case 2:  hipLaunchKernelGGL((mttkrp_flat_generic_kern<V, 2>), grid, block, 0, st, GARGS); break;
      case 3:  hipLaunchKernelGGL((mttkrp_flat_generic_kern<V, 3>), grid, block, 0, st, GARGS); break;
      case 4:  hipLaunchKernelGGL((mttkrp_flat_generic_kern<V, 4>), grid, block, 0, st, GARGS); break;
      case 5:  hipLaunchKernelGGL((mttkrp_flat_generic_kern<V, 5>), grid, block, 0, st, GARGS); break;
      case 6:  hipLaunchKernelGGL((mttkrp_flat_generic_kern<V, 6>), grid, block, 0, st, GARGS); break;
      default: hipLaunchKernelGGL((mttkrp_flat_generic_kern<V, 7>), grid, block, 0, st, GARGS); break;
    }
#undef GARGS
    return true;
  }
  return false;
}

}  // namespace

namespace splatt {
namespace hip {

template <typename V, typename S, typename VS>
int mttkrp_flat(const int32_t * key, const int64_t * rowptr, int64_t nrows,
                int64_t p0, const int32_t * const * idx,
                const S * const * mats, const VS * vals, int64_t nnz, V * out,
                int rank, int nother, void * stream) {
  hipStream_t st = (hipStream_t)stream;
  if (rowptr ? launch_flat7<V, S, VS>(nullptr, rowptr, nrows, p0, idx, mats,
                                      vals, nnz, out, rank, nother, st)
             : launch_flat7<V, S, VS>(key, nullptr, 0, 0, idx, mats, vals,
                                      nnz, out, rank, nother, st))
    return launch_rc();
  // v7 declined. A key stream of V values has the older kernels behind it.
  if constexpr (std::is_same<VS, V>::value) {
    if (!rowptr && launch_flat<V, S>(key, idx, mats, vals, nnz, out, rank,
                                     nother, st))
      return launch_rc();
  }
  return -1;
}

#define FLAT7_SIG(V, S, VS)                                                \
  const int32_t *, const int64_t *, int64_t, int64_t,                      \
  const int32_t * const *, const S * const *, const VS *, int64_t, V *,    \
  int, int
// every type combination the flat family exists in
template int mttkrp_flat<double, double, double>(
    FLAT7_SIG(double, double, double), void *);
template int mttkrp_flat<float, float, float>(
    FLAT7_SIG(float, float, float), void *);
template int mttkrp_flat<double, float, double>(
    FLAT7_SIG(double, float, double), void *);
template int mttkrp_flat<double, bf16, double>(
    FLAT7_SIG(double, bf16, double), void *);
template int mttkrp_flat<double, double, float>(
    FLAT7_SIG(double, double, float), void *);
#undef FLAT7_SIG

}  // namespace hip
}  // namespace splatt
