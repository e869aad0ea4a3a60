// csrc/exact_f32.h -- float arithmetic that rounds as the reference's CPU code does, stated once for every kernel that
// must reproduce one of its decisions bit for bit: each operation rounded on its own (no contraction, whatever the build
// flags say), IEEE divide and square root, and the two orders in which the reference sums three terms.  Device code only;
// no state.
#pragma once

#include <hip/hip_runtime.h>

namespace pgp {
namespace exact {

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 ld3(const float4* __restrict__ a, int i) {
  const float4 v = a[i];
  return {v.x, v.y, v.z};
}

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float fdiv(float a, float b) { return __fdiv_rn(a, b); }

// Correctly rounded float sqrt.  ROCm 7.2's __fsqrt_rn / sqrtf are 1 ulp off for ~15 % of inputs
// on gfx950 (measured: 632 495 of 4 194 304 random values differ from IEEE sqrtf), the double
// square root is exact, and rounding a 53-bit correctly rounded root to 24 bits is innocuous.
__device__ __forceinline__ float sqrt_rn(float z) { return (float)__dsqrt_rn((double)z); }

__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return {sub(a.x, b.x), sub(a.y, b.y), sub(a.z, b.z)}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {sub(mul(a.y, b.z), mul(a.z, b.y)), sub(mul(a.z, b.x), mul(a.x, b.z)), sub(mul(a.x, b.y), mul(a.y, b.x))};
}

// A sum of three terms has two orders, and the reference uses both.  _eigen: a + (b + c), what Eigen's redux makes of a
// 3-vector's dot(), squaredNorm() and norm() (the matcher's PPF key, pair distances, congruent sets, rigid fit).  _lr:
// (a + b) + c, a hand-written x x + y y + z z read left to right (the position-only base selection).  The order is part
// of a function's name so that a call site says which one it reproduces.
__device__ __forceinline__ float sum3_eigen(float a, float b, float c) { return add(a, add(b, c)); }
__device__ __forceinline__ float sum3_lr(float a, float b, float c) { return add(add(a, b), c); }

__device__ __forceinline__ float dot_eigen(V3 a, V3 b) { return sum3_eigen(mul(a.x, b.x), mul(a.y, b.y), mul(a.z, b.z)); }
__device__ __forceinline__ float dot_lr(V3 a, V3 b) { return sum3_lr(mul(a.x, b.x), mul(a.y, b.y), mul(a.z, b.z)); }
__device__ __forceinline__ float sqnorm_eigen(V3 v) { return dot_eigen(v, v); }
__device__ __forceinline__ float sqnorm_lr(V3 v) { return dot_lr(v, v); }
__device__ __forceinline__ float norm_eigen(V3 v) { return sqrt_rn(sqnorm_eigen(v)); }
__device__ __forceinline__ float norm_lr(V3 v) { return sqrt_rn(sqnorm_lr(v)); }

// Eigen normalized(): z = squaredNorm(); z > 0 ? v / sqrt(z) : v
__device__ __forceinline__ V3 normalized(V3 v) {
  const float z = sqnorm_eigen(v);
  if (z > 0.f) {
    const float n = sqrt_rn(z);
    return {fdiv(v.x, n), fdiv(v.y, n), fdiv(v.z, n)};
  }
  return v;
}

// p1 + inv * (p2 - p1)
__device__ __forceinline__ V3 lerp_pt(V3 p1, V3 p2, float inv) {
  const V3 d = vsub(p2, p1);
  return {add(p1.x, mul(inv, d.x)), add(p1.y, mul(inv, d.y)), add(p1.z, mul(inv, d.z))};
}

}  // namespace exact
}  // namespace pgp
