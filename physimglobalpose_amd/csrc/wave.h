// csrc/wave.h -- the cross-lane and four-wave idioms of the kernels, stated once.  Three contracts hold for everything here:
//   1. FULL WAVE.  Every function is called by all 64 lanes of the wave (wave size 64; the shuffles and DPP moves read
//      lanes that must be active).  The block4_* functions are called by all 256 threads of the block.
//   2. FIXED ASSOCIATION.  The order in which values are combined is part of the interface: float and double callers are
//      compared bit for bit against references that add in the same order.
//        reduce / sum / min / max   xor butterfly, offsets 32, 16, 8, 4, 2, 1; at each step v = op(v, value of lane ^ offset).
//                                   Every lane ends with the same value.
//        scan_incl                  __shfl_up, offsets 1, 2, .. 32; lanes >= offset take v = op(v, value of lane - offset)
//        sum_dpp(float)             balanced trees inside the four 16-lane rows, then (r0 + r1) + (r2 + r3)
//        sum_dpp(double)            the same row trees, then ((r0 + r1) + r2) + r3         (NOT the float's order)
//        block4_total               ((s0 op s1) op s2) op s3
//        block4_offset              (((init op s0) op s1) ..) op s[wave - 1]
//   3. FOUR WAVES.  block4_* serve blocks of exactly 256 threads = 4 waves and index the caller's LDS array of 4 entries by
//      the wave number.  Blocks of another shape keep their own tails.
// The __shfl forms go through LDS hardware (ds_bpermute), the DPP forms through the VALU's cross-lane path; a site uses the
// form it was measured with.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pgp {
namespace wave {

__device__ __forceinline__ int lane() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }

// how many set bits of a __ballot belong to lanes below `lane`: the lane's place among the wave's flagged lanes
__device__ __forceinline__ unsigned rank_in(unsigned long long ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

// the operators; float minima and maxima are fminf / fmaxf (the other operand where one is NaN)
struct Add {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct Min {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct Max {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

// ---- reductions by xor butterfly (32- and 64-bit T) ----
template <class T, class Op>
__device__ __forceinline__ T reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
// N values in ONE loop: a shuffle per value per step, so the N round trips overlap
template <class T, int N, class Op>
__device__ __forceinline__ void reduce(T (&v)[N], Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = op(v[k], __shfl_xor(v[k], o, 64));
}
template <class T>
__device__ __forceinline__ T sum(T v) { return reduce(v, Add{}); }
template <class T>
__device__ __forceinline__ T min(T v) { return reduce(v, Min{}); }
template <class T>
__device__ __forceinline__ T max(T v) { return reduce(v, Max{}); }

// ---- inclusive scans ----
template <class T, class Op = Add>
__device__ __forceinline__ T scan_incl(T v, int lane, Op op = Op{}) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(v, off, 64);
    if (lane >= off) v = op(v, o);
  }
  return v;
}

// Inclusive prefix sum over the 64 lanes on the DPP path: a shift-and-add scan inside each 16-lane
// row (zeros are shifted in at the row start), then the row totals are carried across rows
// (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) -- six additions, no LDS.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_scan_step(uint32_t v) {
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
}
__device__ __forceinline__ uint32_t scan_incl_dpp(uint32_t v) {
  v = dpp_scan_step<0x111, 0xF>(v);  // row_shr:1
  v = dpp_scan_step<0x112, 0xF>(v);  // row_shr:2
  v = dpp_scan_step<0x114, 0xF>(v);  // row_shr:4
  v = dpp_scan_step<0x118, 0xF>(v);  // row_shr:8
  v = dpp_scan_step<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  v = dpp_scan_step<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}

// ---- sums on the DPP path, the same value in every lane ----
// float: four row-local steps (quad swaps, half-row and row mirrors -- after them every lane of a 16-lane row holds the
// row total), then the four row totals (r0+r1)+(r2+r3).
template <int CTRL>
__device__ __forceinline__ float dpp_step(float v) {
  const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true);
  return __fadd_rn(v, __int_as_float(moved));
}
__device__ __forceinline__ float sum_dpp(float v) {
  v = dpp_step<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_step<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_step<0x141>(v);  // row_half_mirror
  v = dpp_step<0x140>(v);  // row_mirror
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return __fadd_rn(__fadd_rn(r0, r1), __fadd_rn(r2, r3));
}
// double: the same four steps (two register moves + one v_add_f64 each), then the four row sums are read with v_readlane
// and added in row order, ((r0 + r1) + r2) + r3.  (__shfl_xor on doubles = 12 ds_bpermute round trips per value.)
template <int CTRL>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int plo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  const int phi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  return v + __hiloint2double(phi, plo);
}
__device__ __forceinline__ double sum_dpp(double v) {
  v = dpp_add_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v = dpp_add_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  v = dpp_add_f64<0x141>(v);   // row_half_mirror
  v = dpp_add_f64<0x140>(v);   // row_mirror: every lane of a row holds the row's sum
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const double r0 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
  const double r1 = __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
  const double r2 = __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
  const double r3 = __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
  return ((r0 + r1) + r2) + r3;
}

// ---- the tail of a four-wave block; s is the caller's LDS array of 4 ----
// One lane of each wave (`writer`: lane 0 after a reduction or a ballot, lane 63 after an inclusive scan) leaves its wave's
// value in s[wave], then the block meets: the ONE barrier in here.  Where s still holds an earlier round that some wave may
// be reading, the caller puts a barrier in front.
template <class T, class V>
__device__ __forceinline__ void block4_publish(T* s, bool writer, V v) {
  if (writer) s[wave_id()] = v;
  __syncthreads();
}
// after block4_publish: what the waves in front of `wave` left, folded onto init in wave order
template <class T, class Op = Add>
__device__ __forceinline__ T block4_offset(const T* s, int wave, T init, Op op = Op{}) {
  for (int w = 0; w < wave; ++w) init = op(init, s[w]);
  return init;
}
// after block4_publish: the block's value, ((s0 op s1) op s2) op s3
template <class T, class Op = Add>
__device__ __forceinline__ T block4_total(const T* s, Op op = Op{}) {
  return op(op(op(s[0], s[1]), s[2]), s[3]);
}
// Ordered compaction, after block4_publish of every wave's __popcll(ballot): init + the number of flagged threads in front of
// this one in thread order (meaningful in the flagged threads).  No barrier; block4_total(s) is the block's count.
__device__ __forceinline__ uint32_t block4_rank(const uint32_t* s, unsigned long long ballot, uint32_t init) {
  return block4_offset(s, wave_id(), init + rank_in(ballot, lane()));
}

}  // namespace wave
}  // namespace pgp
