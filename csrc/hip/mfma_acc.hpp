// Operand / accumulator maps of the 16x16x4 MFMA forms on gfx950, shared by
// the Gram kernel (dense_kernels.hip) and the completion row-solve kernel
// (complete_als.hip).
//
// For these shapes the A-operand layout is A[m=lane&15][k=lane>>4] and the
// B-operand layout is B[k=lane>>4][n=lane&15] — mutual transposes — so
// feeding the SAME per-lane value x = chunk[k][col] as both operands
// computes chunk^T * chunk directly.
#pragma once
#include <hip/hip_runtime.h>

template <typename V> struct MfmaAcc;
template <> struct MfmaAcc<double> {
  using type = __attribute__((ext_vector_type(4))) double;
  static __device__ __forceinline__ type mfma(double a, double b, type c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // f64 16x16x4 C/D row map (probed on gfx950): row = lane/16 + 4*reg
  static __device__ __forceinline__ int crow(int lane, int i) {
    return (lane >> 4) + 4 * i;
  }
};
template <> struct MfmaAcc<float> {
  using type = __attribute__((ext_vector_type(4))) float;
  static __device__ __forceinline__ type mfma(float a, float b, type c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // f32 16x16x4 uses the standard map: row = (lane/16)*4 + reg
  static __device__ __forceinline__ int crow(int lane, int i) {
    return (lane >> 4) * 4 + i;
  }
};
