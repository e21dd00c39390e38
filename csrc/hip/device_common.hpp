// Small helpers shared by the kernel files. Everything lives in an
// anonymous namespace (internal linkage, as when each file had its own
// copy), so kernel symbols and generated code do not depend on this header.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>

namespace {

constexpr int WAVE = 64;

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// CDNA has native global fadd for f32/f64; unsafeAtomicAdd emits it (plain
// atomicAdd lowers to a CAS loop without -munsafe-fp-atomics).
template <typename V>
__device__ __forceinline__ void atomic_add_g(V * p, V v) {
  unsafeAtomicAdd(p, v);
}

// streamed-once arrays (key/idx/vals) are loaded non-temporally so they do
// not evict the factor-row working set from the per-XCD L2s
template <typename T>
__device__ __forceinline__ T ldnt(const T * p) {
  return __builtin_nontemporal_load(p);
}

// ranks with a compile-time-F kernel instance (the column-group width)
inline bool spec_ok(int F) {
  return F == 4 || F == 8 || F == 16 || F == 32 || F == 64;
}

// Nonzeros per wave of the flat kernels: enough waves to fill 256 CUs many
// times over, >= 256 nonzeros each. The only reader of SPLATT_SPAN_WAVES
// (tuning knob): the flat launchers and the deterministic workspace size
// (flat_det_ws) must see the same span.
inline int64_t pick_span(int64_t nnz) {
  const char * e = getenv("SPLATT_SPAN_WAVES");
  const int64_t target_waves = e ? atoll(e) : 65536;
  int64_t span = nnz / target_waves;
  if (span < 256) span = 256;
  if (span > 16384) span = 16384;
  return span;
}

// Sub-spans of the flat kernels: [p0, p1) is part `sub` of the `nsub` even
// parts of [lo, hi); false when it is empty. Computed here alone for v2,
// v5, v6 and the key-sorted deterministic pair, whose fixup re-derives every
// walker's range and must agree with the kernel it follows. (det6 and its
// fixup write the same arithmetic out: with this helper their comparisons
// come out mirrored, and their code is kept instruction-identical.)
__device__ __forceinline__ bool sub_range(int64_t lo, int64_t hi, int sub,
                                          int nsub, int64_t & p0,
                                          int64_t & p1) {
  const int64_t gsz = (hi - lo + nsub - 1) / nsub;
  p0 = min64(hi, lo + sub * gsz);
  p1 = min64(hi, p0 + gsz);
  return p0 < p1;
}

// ... of column group g (of R) of wave wid, which covers [wid*span, ..)
__device__ __forceinline__ bool group_range(int64_t wid, int g, int R,
                                            int64_t nnz, int64_t span,
                                            int64_t & p0, int64_t & p1) {
  const int64_t w0 = wid * span;
  if (w0 >= nnz) return false;
  return sub_range(w0, min64(nnz, w0 + span), g, R, p0, p1);
}

// status of the launches just made, in the launcher return convention
// (launchers.hpp): 0 or a positive hipError_t
inline int launch_rc() { return (int)hipGetLastError(); }

}  // namespace
