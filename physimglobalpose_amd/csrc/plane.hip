// csrc/plane.hip -- table-plane removal on gfx950: batched MSAC plane fit and the depth mask.
//
// Replaces pcl::SACSegmentation (SACMODEL_PLANE, SAC_MSAC, threshold 0.005, 1000 iterations, optimised
// coefficients) and the pixel loop of SceneCfg::removeTable (PPE/data_layer/SceneCfg.cpp:38-82); the rules are
// those of include/pgp.h (pgp_fit_plane, pgp_mask_plane_depth).  PCL is not vendored: its bits are not pinned.
//
// Mapping.  Every candidate is scored against every point in ONE pass over (point chunk x candidate block)
// tiles, instead of PCL's one-model-at-a-time loop:
//   plane_candidates  one thread per slot: draw (or read) the triple, the float coefficients, the valid flag
//   plane_score       grid (chunk blocks, candidate blocks of kCb), 256 threads: a thread keeps kPpt points of a
//                     2048-point chunk in registers, the block's kCb coefficient rows sit in LDS (wave-uniform
//                     broadcast reads); per candidate a lane sums its points' min(dist, thr) in double, the wave
//                     folds the 64 lanes with a xor butterfly and counts inliers with a ballot.  A chunk block
//                     walks chunks bx, bx + gridDim.x, ... and adds each chunk's wave sums in that order, so the
//                     workspace holds (candidate, chunk block) partials
//   plane_reduce      one thread per candidate: the partials in chunk-block order (stored [chunk block][candidate])
//   plane_select      one workgroup: valid ranks (sum scan), records (exclusive prefix-min of the penalties,
//                     strict <), k at every record in parallel, the record in force at each rank (max scan), the
//                     first rank where the stop holds (min scan) -- PCL's sequential rule without a serial walk
//   plane_moments / plane_cov / plane_refit   the centroid and covariance of the chosen sample's inliers, per
//                     chunk partials in double, added by one wave in a fixed order, pcl::eigen33 (eigen33.h)
//   plane_inliers     one thread per point: the final plane's strict-< inliers; integer counts per block
// Every floating-point sum has a fixed order: the results are reproducible bit for bit (no float atomics).
//
// Depth mask (plane_mask_depth): one thread per pixel, the reference's loop -- float back-projection, a double
// distance from the float coefficients, dist < threshold zeroes the pixel.

#include "pgp_internal.h"
#include "wave.h"
#include "exact_f32.h"
#include "eigen33.h"

#include <cfloat>
#include <climits>
#include <cmath>

namespace pgp {

namespace {

constexpr int kThreads = 256;
constexpr int kPpt = 8;                          // points per thread in a scoring tile
constexpr int kChunk = kThreads * kPpt;          // 2048 points per chunk
constexpr int kCb = 32;                          // candidates per scoring block (coefficient rows in LDS)
constexpr int kMaxChunkBlocks = 128;             // chunk blocks of the scoring grid (each walks several chunks)
constexpr int kAttempts = 64;                    // draws per slot before it is marked invalid
constexpr int kSelThreads = 1024;
constexpr int kMaxCandidates = 65535;

using exact::sqrt_rn;   // exact_f32.h

__device__ __forceinline__ float plane_dist(float4 q, float x, float y, float z) {
  return fabsf(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q.x, x), __fmul_rn(q.y, y)), __fmul_rn(q.z, z)), q.w));
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;
}

// the coefficients of the plane through three points (include/pgp.h order); false when the cross product is exactly
// zero or its norm does not survive float
__device__ bool plane_of(const float* __restrict__ xyz, int i0, int i1, int i2, float4* out) {
  const float x0 = xyz[3 * (size_t)i0], y0 = xyz[3 * (size_t)i0 + 1], z0 = xyz[3 * (size_t)i0 + 2];
  const float ux = __fsub_rn(xyz[3 * (size_t)i1], x0), uy = __fsub_rn(xyz[3 * (size_t)i1 + 1], y0),
              uz = __fsub_rn(xyz[3 * (size_t)i1 + 2], z0);
  const float vx = __fsub_rn(xyz[3 * (size_t)i2], x0), vy = __fsub_rn(xyz[3 * (size_t)i2 + 1], y0),
              vz = __fsub_rn(xyz[3 * (size_t)i2 + 2], z0);
  const float nx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
  const float ny = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
  const float nz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
  if (nx == 0.f && ny == 0.f && nz == 0.f) return false;
  const float len = sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
  if (!(len > 0.f && len <= FLT_MAX)) return false;
  const float a = __fdiv_rn(nx, len), b = __fdiv_rn(ny, len), c = __fdiv_rn(nz, len);
  const float d = -__fadd_rn(__fadd_rn(__fmul_rn(a, x0), __fmul_rn(b, y0)), __fmul_rn(c, z0));
  *out = make_float4(a, b, c, d);
  return true;
}

// flag bits of the workspace's status word
constexpr int kFlagNonFinite = 1, kFlagBadSample = 2;

__global__ __launch_bounds__(kThreads) void plane_candidates(const float* __restrict__ xyz, int n,
                                                             const int* __restrict__ samples, int m,
                                                             unsigned long long seed, float4* __restrict__ coeff,
                                                             int* __restrict__ valid, int* __restrict__ flag) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  bool ok = false;
  if (samples) {
    const int i0 = samples[3 * (size_t)i], i1 = samples[3 * (size_t)i + 1], i2 = samples[3 * (size_t)i + 2];
    if ((unsigned)i0 < (unsigned)n && (unsigned)i1 < (unsigned)n && (unsigned)i2 < (unsigned)n)
      ok = plane_of(xyz, i0, i1, i2, &q);
    else
      atomicOr(flag, kFlagBadSample);
  } else {
    const unsigned long long st = sample_state(seed, i);
    for (int a = 0; a < kAttempts && !ok; ++a) {
      const int i0 = (int)(sample_variate(st, 3 * a) % (unsigned)n);
      const int i1 = (int)(sample_variate(st, 3 * a + 1) % (unsigned)n);
      const int i2 = (int)(sample_variate(st, 3 * a + 2) % (unsigned)n);
      if (i0 == i1 || i0 == i2 || i1 == i2) continue;
      ok = plane_of(xyz, i0, i1, i2, &q);
    }
  }
  coeff[i] = ok ? q : make_float4(0.f, 0.f, 0.f, 0.f);
  valid[i] = ok ? 1 : 0;
}

// grid (chunk blocks, candidate blocks): partial penalty and inlier count per (candidate, chunk block)
__global__ __launch_bounds__(kThreads) void plane_score(const float* __restrict__ xyz, int n, int n_chunks,
                                                        const float4* __restrict__ coeff, int m, float thr,
                                                        double* __restrict__ pen_part, int* __restrict__ cnt_part,
                                                        int* __restrict__ flag) {
  __shared__ float4 s_q[kCb];
  __shared__ double s_pen[kThreads / 64][kCb];
  __shared__ int s_cnt[kThreads / 64][kCb];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c0 = blockIdx.y * kCb;
  if (t < kCb) {
    s_q[t] = c0 + t < m ? coeff[c0 + t] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int w = 0; w < kThreads / 64; ++w) {
      s_pen[w][t] = 0.0;
      s_cnt[w][t] = 0;
    }
  }
  __syncthreads();
  const int nc = min(kCb, m - c0);
  bool bad = false;
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    float px[kPpt], py[kPpt], pz[kPpt];
    bool in[kPpt];
#pragma unroll
    for (int k = 0; k < kPpt; ++k) {
      const int i = ch * kChunk + k * kThreads + t;
      in[k] = i < n;
      px[k] = in[k] ? xyz[3 * (size_t)i] : 0.f;
      py[k] = in[k] ? xyz[3 * (size_t)i + 1] : 0.f;
      pz[k] = in[k] ? xyz[3 * (size_t)i + 2] : 0.f;
      bad |= in[k] && !finite3(px[k], py[k], pz[k]);
    }
    for (int c = 0; c < nc; ++c) {
      const float4 q = s_q[c];
      double s = 0.0;
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < kPpt; ++k) {
        const float d = plane_dist(q, px[k], py[k], pz[k]);
        s += in[k] ? (double)fminf(d, thr) : 0.0;
        cnt += __popcll(__ballot(in[k] && d <= thr));
      }
      s = wave::sum(s);
      if (lane == 0) {   // chunk order within the wave's own accumulator
        s_pen[wave][c] += s;
        s_cnt[wave][c] += cnt;
      }
    }
  }
  if (bad && blockIdx.y == 0) atomicOr(flag, kFlagNonFinite);
  __syncthreads();
  if (t < nc) {
    const size_t o = (size_t)blockIdx.x * m + (c0 + t);   // [chunk block][candidate]: plane_reduce reads coalesced
    pen_part[o] = ((s_pen[0][t] + s_pen[1][t]) + s_pen[2][t]) + s_pen[3][t];
    cnt_part[o] = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
  }
}

__global__ __launch_bounds__(kThreads) void plane_reduce(const double* __restrict__ pen_part,
                                                         const int* __restrict__ cnt_part, int n_parts, int m,
                                                         const int* __restrict__ valid, double* __restrict__ pen,
                                                         int* __restrict__ cnt) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  double s = 0.0;
  int c = 0;
  for (int b = 0; b < n_parts; ++b) {
    s += pen_part[(size_t)b * m + i];
    c += cnt_part[(size_t)b * m + i];
  }
  pen[i] = valid[i] ? s : __longlong_as_double(0x7FF0000000000000ll);   // an invalid slot never becomes a record
  cnt[i] = c;
}

// Hillis-Steele inclusive scan over the workgroup; `s` is kSelThreads entries of LDS
template <class T, class Op>
__device__ T block_scan(T v, T* s, Op op) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < kSelThreads; off <<= 1) {
    const T o = t >= off ? s[t - off] : v;
    __syncthreads();
    if (t >= off) v = op(o, v);
    s[t] = v;
    __syncthreads();
  }
  return v;
}

struct SelArgs {
  const double* pen;
  const int* cnt;
  const int* valid;
  const float4* coeff;
  int m, n, max_it, stop;
  double log_p;
  const int* flag;
  int* chosen;            // workspace: the chosen slot (-1: none)
  float4* plane;          // workspace: the plane the refit starts from
  pgp_plane_info* info;   // nullable
};

__global__ __launch_bounds__(kSelThreads) void plane_select(SelArgs a) {
  __shared__ double s_d[kSelThreads];
  __shared__ int s_i[kSelThreads];
  __shared__ double s_k[kSelThreads];
  __shared__ int s_res[2];
  const int t = threadIdx.x;
  const bool adaptive = a.stop == PGP_PLANE_STOP_ADAPTIVE;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  const double inv_n = 1.0 / (double)a.n;
  double best = inf, k_carry = 1.0;   // PCL starts with k = 1
  int ranks = 0, last_rec = -1;
  if (t == 0) s_res[0] = s_res[1] = -1;
  bool done = false;
  for (int base = 0; base < a.m && !done; base += kSelThreads) {
    const int j = base + t;
    const int v = j < a.m ? a.valid[j] : 0;
    const double p = v ? a.pen[j] : inf;
    const int e = block_scan(v, s_i, [](int x, int y) { return x + y; }) + ranks;
    const int tile_valid = s_i[kSelThreads - 1];
    block_scan(p, s_d, [](double x, double y) { return fmin(x, y); });
    const double before = t == 0 ? best : fmin(best, s_d[t - 1]);
    const double tile_min = s_d[kSelThreads - 1];
    const bool rec = v && p < before;
    double k = 0.0;
    if (rec && adaptive) {   // k = log(1 - p) / log(1 - w^3), clamped as PCL clamps it
      const double w = (double)a.cnt[j] * inv_n;
      double pno = 1.0 - pow(w, 3.0);
      pno = fmax(DBL_EPSILON, pno);
      pno = fmin(1.0 - DBL_EPSILON, pno);
      k = a.log_p / log(pno);
    }
    s_k[t] = k;
    const int lr = max(block_scan(rec ? j : -1, s_i, [](int x, int y) { return max(x, y); }), last_rec);
    const int tile_lr = max(s_i[kSelThreads - 1], last_rec);
    bool stop = false;
    if (adaptive && v) {
      const double kc = lr < 0 ? 1.0 : (lr >= base ? s_k[lr - base] : k_carry);
      stop = (double)e >= kc || e > a.max_it;
    }
    const int first = block_scan(stop ? j : INT_MAX, s_i, [](int x, int y) { return min(x, y); });
    const int tile_first = s_i[kSelThreads - 1];
    (void)first;
    if (tile_first != INT_MAX) {
      if (j == tile_first) {
        s_res[0] = lr;
        s_res[1] = e;
      }
      done = true;
    } else {
      if (tile_lr >= base) k_carry = s_k[tile_lr - base];
      last_rec = tile_lr;
      best = fmin(best, tile_min);
      ranks += tile_valid;
    }
    __syncthreads();
  }
  // every valid slot, whatever the stop
  int nv = 0;
  for (int j = t; j < a.m; j += kSelThreads) nv += a.valid[j];
  nv = block_scan(nv, s_i, [](int x, int y) { return x + y; });
  nv = s_i[kSelThreads - 1];
  if (t != 0) return;
  int chosen = done ? s_res[0] : last_rec;
  int n_eval = done ? s_res[1] : ranks;
  const int fl = *a.flag;
  if (fl) {
    chosen = -1;
    n_eval = 0;
  }
  const float4 q = chosen >= 0 ? a.coeff[chosen] : make_float4(0.f, 0.f, 0.f, 0.f);
  *a.chosen = chosen;
  *a.plane = q;
  if (a.info) {
    pgp_plane_info r;
    r.status = fl ? PGP_EINVAL : PGP_OK;
    r.chosen = chosen;
    r.n_evaluated = n_eval;
    r.n_valid = fl ? 0 : nv;
    r.n_candidates = a.m;
    r.sampled_inliers = chosen >= 0 ? a.cnt[chosen] : 0;
    r.penalty = chosen >= 0 ? a.pen[chosen] : 0.0;
    r.sampled[0] = q.x;
    r.sampled[1] = q.y;
    r.sampled[2] = q.z;
    r.sampled[3] = q.w;
    *a.info = r;
  }
}

// the workgroup's sum in a fixed order: lanes by the xor butterfly, then waves 0..3
__device__ __forceinline__ double block_sum_d(double v, double* s_w) {
  v = wave::sum(v);
  __syncthreads();   // s_w may still be read from the call before
  wave::block4_publish(s_w, wave::lane() == 0, v);
  return wave::block4_total(s_w);   // ((s0 + s1) + s2) + s3
}

// refit pass 1: per chunk, {count, sum x, sum y, sum z} of the chosen sample's strict inliers
__global__ __launch_bounds__(kThreads) void plane_moments(const float* __restrict__ xyz, int n, float thr,
                                                          const int* __restrict__ chosen, const float4* __restrict__ plane,
                                                          double* __restrict__ part) {
  __shared__ double s_w[kThreads / 64];
  const float4 q = *plane;
  const bool on = *chosen >= 0;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < kPpt && on; ++k) {
    const int i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    if (i >= n) break;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    if (plane_dist(q, x, y, z) < thr) {
      acc[0] += 1.0;
      acc[1] += (double)x;
      acc[2] += (double)y;
      acc[3] += (double)z;
    }
  }
  for (int c = 0; c < 4; ++c) {
    const double s = block_sum_d(acc[c], s_w);
    if (threadIdx.x == 0) part[4 * (size_t)blockIdx.x + c] = s;
  }
}

// the sum of K-vector partials over chunks by ONE wave, in a fixed order: lane l adds chunks l, l + 64, ... in turn,
// the lanes fold by the xor butterfly (every lane ends with the same sums)
template <int K>
__device__ __forceinline__ void wave_sum_parts(const double* __restrict__ part, int n_chunks, double out[K]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.0;
  for (int b = lane; b < n_chunks; b += 64)
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] += part[K * (size_t)b + k];
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = wave::sum(out[k]);
}

// {count, centroid}: run by a whole wave
__device__ __forceinline__ void centroid_of(const double* __restrict__ part, int n_chunks, double c[4]) {
  wave_sum_parts<4>(part, n_chunks, c);
  if (c[0] > 0.0)
    for (int k = 1; k < 4; ++k) c[k] /= c[0];
}

// refit pass 2: per chunk, the six covariance sums about the centroid
__global__ __launch_bounds__(kThreads) void plane_cov(const float* __restrict__ xyz, int n, float thr,
                                                      const int* __restrict__ chosen, const float4* __restrict__ plane,
                                                      const double* __restrict__ part4, int n_chunks,
                                                      double* __restrict__ part6) {
  __shared__ double s_w[kThreads / 64];
  __shared__ double s_c[4];
  if (threadIdx.x < 64) {
    double c[4];
    centroid_of(part4, n_chunks, c);
    if (threadIdx.x == 0)
      for (int k = 0; k < 4; ++k) s_c[k] = c[k];
  }
  __syncthreads();
  const float4 q = *plane;
  const bool on = *chosen >= 0;
  const double cx = s_c[1], cy = s_c[2], cz = s_c[3];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < kPpt && on; ++k) {
    const int i = blockIdx.x * kChunk + k * kThreads + threadIdx.x;
    if (i >= n) break;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    if (plane_dist(q, x, y, z) < thr) {
      const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
      acc[0] += dx * dx;
      acc[1] += dx * dy;
      acc[2] += dx * dz;
      acc[3] += dy * dy;
      acc[4] += dy * dz;
      acc[5] += dz * dz;
    }
  }
  for (int c = 0; c < 6; ++c) {
    const double s = block_sum_d(acc[c], s_w);
    if (threadIdx.x == 0) part6[6 * (size_t)blockIdx.x + c] = s;
  }
}

__global__ __launch_bounds__(64) void plane_refit(const double* __restrict__ part4, const double* __restrict__ part6,
                                                  int n_chunks, const int* __restrict__ chosen, float4* __restrict__ plane) {
  if (*chosen < 0) return;
  double c[4], cov[6];
  centroid_of(part4, n_chunks, c);
  wave_sum_parts<6>(part6, n_chunks, cov);
  if (threadIdx.x != 0 || c[0] < 3.0) return;   // fewer than 3 inliers: the sampled plane stays
  double ev, nrm[3];
  eigen33_smallest(cov, &ev, nrm);
  if (!(fabs(nrm[0]) <= 1.0 && fabs(nrm[1]) <= 1.0 && fabs(nrm[2]) <= 1.0)) return;   // NaN: keep the sample
  const double d = -((nrm[0] * c[1] + nrm[1] * c[2]) + nrm[2] * c[3]);
  *plane = make_float4((float)nrm[0], (float)nrm[1], (float)nrm[2], (float)d);
}

// the final plane's strict inliers; block counts added with one integer atomic per block
__global__ __launch_bounds__(kThreads) void plane_inliers(const float* __restrict__ xyz, int n, float thr,
                                                          const int* __restrict__ chosen, const float4* __restrict__ plane,
                                                          unsigned char* __restrict__ mask, int* __restrict__ n_inl,
                                                          float* __restrict__ out_coeff) {
  __shared__ int s_n[kThreads / 64];
  const bool on = *chosen >= 0;
  const float4 q = on ? *plane : make_float4(0.f, 0.f, 0.f, 0.f);
  const int i = blockIdx.x * kThreads + threadIdx.x;
  bool in = false;
  if (i < n) {
    in = on && plane_dist(q, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]) < thr;
    if (mask) mask[i] = in ? 1 : 0;
  }
  const unsigned long long b = __ballot(in);
  wave::block4_publish(s_n, wave::lane() == 0, __popcll(b));
  if (threadIdx.x == 0) {
    const int s = wave::block4_total(s_n);
    if (s) atomicAdd(n_inl, s);
    if (blockIdx.x == 0) {
      out_coeff[0] = q.x;
      out_coeff[1] = q.y;
      out_coeff[2] = q.z;
      out_coeff[3] = q.w;
    }
  }
}

template <bool RAW16>
__global__ __launch_bounds__(kThreads) void plane_mask_depth(void* __restrict__ img, int rows, int cols, float fx,
                                                             float fy, float cx, float cy, float4 q,
                                                             const float* __restrict__ dq, double thr,
                                                             int* __restrict__ n_masked) {
  if (dq) q = make_float4(dq[0], dq[1], dq[2], dq[3]);   // the plane a queued fit leaves in device memory
  __shared__ int s_n[kThreads / 64];
  const size_t n = (size_t)rows * cols;
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  bool hit = false;
  if (i < n) {
    float depth;
    if (RAW16) {
      unsigned short s = static_cast<const unsigned short*>(img)[i];
      s = (unsigned short)((s << 13) | (s >> 3));   // the decode of pgp_backproject_depth (utilities.cpp:57-59)
      depth = __fdiv_rn((float)s, 10000.0f);
    } else {
      depth = static_cast<const float*>(img)[i];
    }
    const int u = (int)(i / (size_t)cols), v = (int)(i - (size_t)u * cols);
    const float x = __fdiv_rn(__fmul_rn(__fsub_rn((float)v, cx), depth), fx);
    const float y = __fdiv_rn(__fmul_rn(__fsub_rn((float)u, cy), depth), fy);
    // pcl::pointToPlaneDistance: |a x + b y + c z + d| with double coefficients
    const double dist = fabs((((double)q.x * (double)x + (double)q.y * (double)y) + (double)q.z * (double)depth) +
                             (double)q.w);
    hit = dist < thr;
    if (hit) {
      if (RAW16) static_cast<unsigned short*>(img)[i] = 0;
      else static_cast<float*>(img)[i] = 0.f;
    }
  }
  if (!n_masked) return;
  const unsigned long long b = __ballot(hit);
  wave::block4_publish(s_n, wave::lane() == 0, __popcll(b));
  if (threadIdx.x == 0) {
    const int s = wave::block4_total(s_n);
    if (s) atomicAdd(n_masked, s);
  }
}

struct PlaneLayout {
  size_t coeff, valid, pen_part, cnt_part, pen, cnt, part4, part6, chosen, plane, flag, total;
};

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

PlaneLayout plane_layout(int n, int m, int n_parts) {
  const size_t M = (size_t)m, nch = (size_t)((n + kChunk - 1) / kChunk);
  PlaneLayout L;
  size_t o = 0;
  L.coeff = o; o += up256(M * sizeof(float4));
  L.valid = o; o += up256(M * 4);
  L.pen_part = o; o += up256(M * (size_t)n_parts * 8);
  L.cnt_part = o; o += up256(M * (size_t)n_parts * 4);
  L.pen = o; o += up256(M * 8);
  L.cnt = o; o += up256(M * 4);
  L.part4 = o; o += up256(nch * 4 * 8);
  L.part6 = o; o += up256(nch * 6 * 8);
  L.chosen = o; o += 256;
  L.plane = o; o += 256;
  L.flag = o; o += 256;
  L.total = o;
  return L;
}

}  // namespace

int plane_max_candidates() { return kMaxCandidates; }

int launch_fit_plane(pgp_ctx* ctx, const float* d_xyz, int n, const pgp_plane_options* opt, const int* d_samples,
                     int n_samples, float* d_coeff, unsigned char* d_inliers, int* d_n_inliers, pgp_plane_info* d_info,
                     hipStream_t st) {
  const int m = d_samples ? n_samples : opt->max_iterations + 1;
  const int n_chunks = (n + kChunk - 1) / kChunk;
  const int n_parts = n_chunks < kMaxChunkBlocks ? n_chunks : kMaxChunkBlocks;
  const PlaneLayout L = plane_layout(n, m, n_parts);
  int rc = ctx->d_plane_ws.ensure(L.total);
  if (rc != PGP_OK) return rc;
  unsigned char* w = ctx->d_plane_ws.as<unsigned char>();
  float4* coeff = reinterpret_cast<float4*>(w + L.coeff);
  int* valid = reinterpret_cast<int*>(w + L.valid);
  double* pen_part = reinterpret_cast<double*>(w + L.pen_part);
  int* cnt_part = reinterpret_cast<int*>(w + L.cnt_part);
  double* pen = reinterpret_cast<double*>(w + L.pen);
  int* cnt = reinterpret_cast<int*>(w + L.cnt);
  double* part4 = reinterpret_cast<double*>(w + L.part4);
  double* part6 = reinterpret_cast<double*>(w + L.part6);
  int* chosen = reinterpret_cast<int*>(w + L.chosen);
  float4* plane = reinterpret_cast<float4*>(w + L.plane);
  int* flag = reinterpret_cast<int*>(w + L.flag);
  PGP_HIP(hipMemsetAsync(flag, 0, 4, st));
  PGP_HIP(hipMemsetAsync(d_n_inliers, 0, 4, st));
  const float thr = opt->threshold;
  hipLaunchKernelGGL(plane_candidates, dim3((m + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d_xyz, n, d_samples, m,
                     opt->seed, coeff, valid, flag);
  hipLaunchKernelGGL(plane_score, dim3(n_parts, (m + kCb - 1) / kCb), dim3(kThreads), 0, st, d_xyz, n, n_chunks,
                     (const float4*)coeff, m, thr, pen_part, cnt_part, flag);
  hipLaunchKernelGGL(plane_reduce, dim3((m + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (const double*)pen_part,
                     (const int*)cnt_part, n_parts, m, (const int*)valid, pen, cnt);
  SelArgs a{pen, cnt, valid, coeff, m, n, opt->max_iterations, opt->stop, log(1.0 - opt->probability), flag, chosen, plane,
            d_info};
  hipLaunchKernelGGL(plane_select, dim3(1), dim3(kSelThreads), 0, st, a);
  if (opt->optimize) {
    hipLaunchKernelGGL(plane_moments, dim3(n_chunks), dim3(kThreads), 0, st, d_xyz, n, thr, (const int*)chosen,
                       (const float4*)plane, part4);
    hipLaunchKernelGGL(plane_cov, dim3(n_chunks), dim3(kThreads), 0, st, d_xyz, n, thr, (const int*)chosen,
                       (const float4*)plane, (const double*)part4, n_chunks, part6);
    hipLaunchKernelGGL(plane_refit, dim3(1), dim3(64), 0, st, (const double*)part4, (const double*)part6, n_chunks,
                       (const int*)chosen, plane);
  }
  hipLaunchKernelGGL(plane_inliers, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d_xyz, n, thr,
                     (const int*)chosen, (const float4*)plane, d_inliers, d_n_inliers, d_coeff);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

// coeff: host coefficients, or d_coeff (non-null): the 4 device floats a queued fit writes
int launch_mask_plane_depth(pgp_ctx* ctx, void* d_img, bool raw16, int rows, int cols, const float K[9],
                            const float* coeff, const float* d_coeff, double thr, int* d_n_masked, hipStream_t st) {
  (void)ctx;
  const size_t n = (size_t)rows * cols;
  if (d_n_masked) PGP_HIP(hipMemsetAsync(d_n_masked, 0, 4, st));
  if (n == 0) return PGP_OK;
  const float4 q = d_coeff ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(coeff[0], coeff[1], coeff[2], coeff[3]);
  const dim3 g((unsigned)((n + kThreads - 1) / kThreads));
  if (raw16)
    hipLaunchKernelGGL(plane_mask_depth<true>, g, dim3(kThreads), 0, st, d_img, rows, cols, K[0], K[4], K[2], K[5], q, d_coeff,
                       thr, d_n_masked);
  else
    hipLaunchKernelGGL(plane_mask_depth<false>, g, dim3(kThreads), 0, st, d_img, rows, cols, K[0], K[4], K[2], K[5], q, d_coeff,
                       thr, d_n_masked);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

}  // namespace pgp
