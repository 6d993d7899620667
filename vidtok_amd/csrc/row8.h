// 8 consecutive channels <-> fp32: one 16-byte access in a 16-bit type, two in fp32 (the row access of the LPIPS kernels, lpips.hip
// and lpips_grad.hip: 8 channels a lane)
#pragma once
#include "common.h"

template <typename T>
struct Row8;
template <>
struct Row8<float> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[8]) {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = v[e]; b[e] = v[4 + e]; }
    *reinterpret_cast<f32x4*>(p) = a;
    *reinterpret_cast<f32x4*>(p + 4) = b;
  }
};
template <typename H>
struct Row8H {
  static __device__ __forceinline__ void load(const H* p, float (&v)[8]) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = h16<H>::lo(w[e]); v[2 * e + 1] = h16<H>::hi(w[e]); }
  }
  static __device__ __forceinline__ void store(H* p, const float (&v)[8]) {
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = h16<H>::pack(v[2 * e], v[2 * e + 1]);
    *reinterpret_cast<u32x4*>(p) = w;
  }
};
template <>
struct Row8<bf16_t> : Row8H<bf16_t> {};
template <>
struct Row8<f16_t> : Row8H<f16_t> {};
