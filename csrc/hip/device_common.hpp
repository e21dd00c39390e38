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

// status of the launches just made, in the launcher return convention
// (launchers.hpp): 0 or a positive hipError_t
inline int launch_rc() { return (int)hipGetLastError(); }

}  // namespace
