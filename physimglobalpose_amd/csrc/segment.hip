// csrc/segment.hip -- the steps between the segment's normals and the scene index, on device arrays:
//
//   radius filter     pcl::RadiusOutlierRemoval + flipNormalTowardsViewpoint + re-normalisation in
//                     CongruentSetMatching::generate (PPE/hypothesis_generation/ObjectPoseCandidateSet.cpp:28-51):
//                     the keep decision on count_neighbours' counts, the flip and the compaction -- what the host form
//                     pgp_radius_outlier_filter leaves to a host loop and to its caller.
//   centring          Match4PCSBase::init, S4/algorithms/match4pcsBase.cc:242-264, for one cloud: centroid += pos in
//                     index order in float, / (float)n, every point minus the centroid.
//   weights           the priority weights of base.cc:317-340: the probability image at each point's pixel.
//
// Mapping.  Filter: an ordered compaction in backproject.hip's shape -- a pass that counts the kept points of each
// workgroup (the kept flag of a wave from __ballot, 64 bits, and __popcll), an exclusive scan of those counts as launches
// of their own, and the same pass again writing behind the scanned offsets; rows leave in input order.  Centring: the
// float sum has ONE order that gives the reference's bits, so one lane adds, three independent chains (x, y, z); the
// other 255 lanes of its workgroup stage the cloud through LDS in chunks so that the adding lane never waits for HBM.
// A second launch subtracts.  Weights: one thread per point.  No kernel waits for another workgroup.
//
// Every float operation that decides a bit is spelled with the _rn intrinsics (no contraction whatever the flags say);
// the square root is exact_f32.h's (the double root rounded once).

#include "pgp_internal.h"
#include "wave.h"
#include "exact_f32.h"

namespace pgp {

namespace {

using exact::sqrt_rn;

constexpr int kSegThreads = 256;

struct FilterArgs {
  const int* counts;     // [n] neighbours within the radius, the point itself included
  const float* xyz;      // n x 3
  const float* nrm;      // n x 3, nullable
  int n;
  int min_neighbors;
  uint32_t* block_ctr;   // [blocks + 1]: kept per workgroup, then their exclusive scan
  float* out_xyz;        // cap x 3
  float* out_nrm;        // cap x 3, nullable
  int* out_index;        // cap, nullable
  uint32_t cap;
};

// pass 1: kept points per workgroup; pass 2 (WRITE): ranked write behind the scanned offsets
template <bool WRITE>
__global__ __launch_bounds__(kSegThreads) void filter_compact(FilterArgs a) {
  __shared__ uint32_t s_wave[kSegThreads / 64];
  const int i = blockIdx.x * kSegThreads + threadIdx.x;
  const bool keep = i < a.n && a.counts[i] > a.min_neighbors;   // PCL 1.7: `k <= min_pts_radius_` -> outlier
  const unsigned long long b = __ballot(keep);
  wave::block4_publish(s_wave, wave::lane() == 0, (uint32_t)__popcll(b));
  if (!WRITE) {
    if (threadIdx.x == 0) a.block_ctr[blockIdx.x] = wave::block4_total(s_wave);
    return;
  }
  if (!keep) return;
  const uint32_t rank = wave::block4_rank(s_wave, b, a.block_ctr[blockIdx.x]);
  if (rank >= a.cap) return;
  const float px = a.xyz[3 * (size_t)i], py = a.xyz[3 * (size_t)i + 1], pz = a.xyz[3 * (size_t)i + 2];
  a.out_xyz[3 * (size_t)rank] = px;
  a.out_xyz[3 * (size_t)rank + 1] = py;
  a.out_xyz[3 * (size_t)rank + 2] = pz;
  if (a.out_index) a.out_index[rank] = i;
  if (a.nrm && a.out_nrm) {
    // pcl::flipNormalTowardsViewpoint(p, 0,0,0, n): flip when (vp - p).n < 0, then / magnitude (a zero normal: NaN)
    float nx = a.nrm[3 * (size_t)i], ny = a.nrm[3 * (size_t)i + 1], nz = a.nrm[3 * (size_t)i + 2];
    const float vx = __fsub_rn(0.f, px), vy = __fsub_rn(0.f, py), vz = __fsub_rn(0.f, pz);
    const float cos_theta = __fadd_rn(__fadd_rn(__fmul_rn(vx, nx), __fmul_rn(vy, ny)), __fmul_rn(vz, nz));
    if (cos_theta < 0.f) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    const float mag = sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
    a.out_nrm[3 * (size_t)rank] = __fdiv_rn(nx, mag);
    a.out_nrm[3 * (size_t)rank + 1] = __fdiv_rn(ny, mag);
    a.out_nrm[3 * (size_t)rank + 2] = __fdiv_rn(nz, mag);
  }
}

// centroid += pos (index order, float), then / (float)n: ONE workgroup; every lane stages, lane 0 adds
constexpr int kChunk = 1024;   // points per LDS chunk (12 KB)

__global__ __launch_bounds__(kSegThreads) void centroid_in_order(const float* __restrict__ xyz, int n,
                                                                 float* __restrict__ centroid) {
  __shared__ float s_p[3 * kChunk];
  float cx = 0.f, cy = 0.f, cz = 0.f;
  for (int base = 0; base < n; base += kChunk) {
    const int m = min(kChunk, n - base);
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * m; j += kSegThreads) s_p[j] = xyz[3 * (size_t)base + j];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 8
      for (int j = 0; j < m; ++j) {
        cx = __fadd_rn(cx, s_p[3 * j]);
        cy = __fadd_rn(cy, s_p[3 * j + 1]);
        cz = __fadd_rn(cz, s_p[3 * j + 2]);
      }
    }
  }
  if (threadIdx.x == 0) {
    const float fn = (float)n;
    centroid[0] = __fdiv_rn(cx, fn);
    centroid[1] = __fdiv_rn(cy, fn);
    centroid[2] = __fdiv_rn(cz, fn);
  }
}

// every point minus c: the centroid the launch in front left on the device (d_c), or a vector given by value
__global__ __launch_bounds__(kSegThreads) void subtract_vector(float* __restrict__ xyz, int n, const float* __restrict__ d_c,
                                                               float sx, float sy, float sz) {
  const int i = blockIdx.x * kSegThreads + threadIdx.x;
  if (i >= n) return;
  if (d_c) {
    sx = d_c[0];
    sy = d_c[1];
    sz = d_c[2];
  }
  xyz[3 * (size_t)i] = __fsub_rn(xyz[3 * (size_t)i], sx);
  xyz[3 * (size_t)i + 1] = __fsub_rn(xyz[3 * (size_t)i + 1], sy);
  xyz[3 * (size_t)i + 2] = __fsub_rn(xyz[3 * (size_t)i + 2], sz);
}

struct PixelArgs {
  float c[3];   // centroid_P
  float K[9];   // row-major intrinsics
  int rows, cols;
};

// image_pixel of pgp_api.hip (base.cc:317-340) per thread, then (float)img / 10000; outside the image: weight 0
__global__ __launch_bounds__(kSegThreads) void weights_from_image(const float* __restrict__ xyz, int n, PixelArgs a,
                                                                  const unsigned short* __restrict__ img,
                                                                  float* __restrict__ weights) {
  const int i = blockIdx.x * kSegThreads + threadIdx.x;
  if (i >= n) return;
  const float x = __fadd_rn(xyz[3 * (size_t)i], a.c[0]), y = __fadd_rn(xyz[3 * (size_t)i + 1], a.c[1]),
              z = __fadd_rn(xyz[3 * (size_t)i + 2], a.c[2]);
  float u[3];
  for (int r = 0; r < 3; ++r)   // Eigen's 3x3 * 3x1: k0 x + (k1 y + k2 z)
    u[r] = __fadd_rn(__fmul_rn(a.K[3 * r], x), __fadd_rn(__fmul_rn(a.K[3 * r + 1], y), __fmul_rn(a.K[3 * r + 2], z)));
  const float fc = __fdiv_rn(u[0], u[2]), fr = __fdiv_rn(u[1], u[2]);
  float w = 0.f;
  if (fc == fc && fr == fr && fc > -1.f && fr > -1.f && fc < (float)a.cols && fr < (float)a.rows) {
    const int col = (int)fc, row = (int)fr;   // truncation toward zero
    if (col >= 0 && row >= 0 && col < a.cols && row < a.rows)
      w = __fdiv_rn((float)img[(size_t)row * a.cols + col], 10000.0f);
  }
  weights[i] = w;
}

}  // namespace

// The index of the cloud itself with delta = radius is the resident scene from here on (as the host form leaves it).
// d_seg_ws: counts [n] | per-workgroup counters [blocks + 1] | scan scratch.  Synchronises `st` for the count.
int launch_radius_filter(pgp_ctx* ctx, const float* d_xyz, const float* d_nrm, int n, float radius, int min_neighbors,
                         float* d_out_xyz, float* d_out_nrm, int* d_out_index, int cap, int* n_kept, hipStream_t st) {
  *n_kept = 0;
  if (n <= 0) return PGP_OK;
  int rc = set_scene_device(ctx, d_xyz, nullptr, nullptr, n, radius, st);
  if (rc != PGP_OK) return rc;
  const int nb = (n + kSegThreads - 1) / kSegThreads;
  Carve lay;
  const auto p_counts = lay.add<int>((size_t)n, 256);
  const auto p_ctr = lay.add<uint32_t>((size_t)nb + 1, 256);
  const auto p_scan = lay.add<uint32_t>((size_t)(nb + 1) / 2048 + 4, 256);
  if ((rc = lay.ensure(ctx->d_seg_ws)) != PGP_OK) return rc;
  int* d_counts = lay.at(p_counts);
  uint32_t* d_ctr = lay.at(p_ctr);
  if ((rc = launch_count_neighbours(ctx, radius, d_counts, st)) != PGP_OK) return rc;
  const FilterArgs a{d_counts, d_xyz, d_nrm, n, min_neighbors, d_ctr, d_out_xyz, d_out_nrm, d_out_index,
                     (uint32_t)(cap > 0 ? cap : 0)};
  PGP_HIP(hipMemsetAsync(d_ctr + nb, 0, sizeof(uint32_t), st));   // scan sentinel
  hipLaunchKernelGGL(filter_compact<false>, dim3(nb), dim3(kSegThreads), 0, st, a);
  if ((rc = device_exclusive_scan(d_ctr, d_ctr, (size_t)nb + 1, lay.at(p_scan), st)) != PGP_OK) return rc;
  hipLaunchKernelGGL(filter_compact<true>, dim3(nb), dim3(kSegThreads), 0, st, a);
  PGP_HIP(hipGetLastError());
  uint32_t total = 0;
  PGP_HIP(hipMemcpyAsync(&total, d_ctr + nb, sizeof total, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  *n_kept = (int)total;
  return PGP_OK;
}

// d_centroid: 3 device floats (nullable: the shift is `shift`, by value).  Enqueued on `st`.
int launch_center(float* d_xyz, int n, float* d_centroid, const float shift[3], hipStream_t st) {
  if (n <= 0) return PGP_OK;
  if (d_centroid) hipLaunchKernelGGL(centroid_in_order, dim3(1), dim3(kSegThreads), 0, st, (const float*)d_xyz, n, d_centroid);
  hipLaunchKernelGGL(subtract_vector, dim3((n + kSegThreads - 1) / kSegThreads), dim3(kSegThreads), 0, st, d_xyz, n,
                     (const float*)d_centroid, shift ? shift[0] : 0.f, shift ? shift[1] : 0.f, shift ? shift[2] : 0.f);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

int launch_weights_from_image(const float* d_xyz, int n, const float c[3], const float K[9], const unsigned short* d_img,
                              int rows, int cols, float* d_weights, hipStream_t st) {
  if (n <= 0) return PGP_OK;
  PixelArgs a{};
  for (int k = 0; k < 3; ++k) a.c[k] = c[k];
  for (int k = 0; k < 9; ++k) a.K[k] = K[k];
  a.rows = rows;
  a.cols = cols;
  hipLaunchKernelGGL(weights_from_image, dim3((n + kSegThreads - 1) / kSegThreads), dim3(kSegThreads), 0, st, d_xyz, n, a,
                     d_img, d_weights);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

}  // namespace pgp
