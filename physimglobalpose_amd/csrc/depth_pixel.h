// csrc/depth_pixel.h -- one depth pixel as the reference reads it: decode, validity, back-projection.  Shared by
// backproject.hip (the cloud) and components.hip (the labelling), so that both see the same pixels and the same bits.
//   utilities::readDepthImage        PPE/misc/utilities.cpp:47-61   raw 16-bit -> metres
//   utilities::convert3dUnOrganized  PPE/misc/utilities.cpp:190-206
#pragma once

#include <hip/hip_runtime.h>

namespace pgp {

template <bool RAW16>
__device__ __forceinline__ float depth_at(const void* img, size_t i) {
  if (RAW16) {
    unsigned short s = static_cast<const unsigned short*>(img)[i];
    s = (unsigned short)((s << 13) | (s >> 3));  // utilities.cpp:57 (APC encoding)
    return __fdiv_rn((float)s, 10000.0f);        // :59 (float)depthShort/10000
  }
  return static_cast<const float*>(img)[i];
}

__device__ __forceinline__ bool depth_ok(float d, double z_min, double z_max) {
  return (double)d > z_min && (double)d < z_max;  // utilities.cpp:197 / :218
}

// x = (v - cx) * depth / fx, y = (u - cy) * depth / fy, z = depth: every operation in float, in that order
__device__ __forceinline__ float3 depth_point(int u, int v, float d, float fx, float fy, float cx, float cy) {
  return make_float3(__fdiv_rn(__fmul_rn(__fsub_rn((float)v, cx), d), fx), __fdiv_rn(__fmul_rn(__fsub_rn((float)u, cy), d), fy),
                     d);
}

}  // namespace pgp
