// csrc/depth_crease.hip -- touching objects cut apart on gfx950: surface normals of the organised depth image, the
// concave-crease test between pixels a few steps apart (the local-convexity criterion of LCCP, Stein et al. 2014, on the
// image grid as in Tateno et al. 2015), and the Jacobi passes that hand the crease pixels back to the cores they separate.
// The rules are those of include/pgp.h (pgp_depth_normals, pgp_depth_crease_mask, pgp_depth_objects); the cores
// themselves are components.hip's labelling, run with the keep bytes as its mask.  The reference has no such step.
//
// Mapping.  All three stencil kernels walk components.hip's kTw x kTh tiles with 256 threads and keep what the stencil
// reads in LDS, one float array per coordinate (a wave reads 64 consecutive words: no bank conflict).  An invalid pixel
// and a pixel outside the image are NaN points, a pixel without a normal is a NaN normal: NaN fails the distance test,
// so "reachable" needs no flag of its own.  LDS is sized by the options at launch (dynamic), not by their maxima.
//   dn_normals  points of the tile + a halo of s + w (back-projected once per pixel), raw normals of the tile + w from
//               them, then the (2 w + 1)^2 window sum in the contract's order (du outer, dv inner) and one float4 out.
//               At the maxima (s 8, w 4): (64 + 24) x (16 + 24) points + 72 x 24 raw normals = 61.5 KiB; at the defaults
//               38 KiB, four workgroups to a CU.
//   dn_crease   points and smoothed normals of the tile + a halo of c, the eight pairs, one keep byte per pixel; the
//               crease count is one ballot per wave and one integer atomic per workgroup.
//   dn_grow     one launch per pass, one thread per pixel, ping-pong id images: a pixel with id 0 reads its four
//               neighbours' ids of the previous pass.  Always all passes: nothing is read home.
// No kernel waits for another workgroup, there is no cooperative launch and no float atomic.

#include "pgp_internal.h"
#include "wave.h"
#include "depth_pixel.h"
#include "exact_f32.h"

#include <climits>

namespace pgp {

namespace {

constexpr int kThreads = 256;
constexpr int kTw = 64, kTh = 16;   // components.hip's tile

struct Cam {
  float fx, fy, cx, cy;
  double z_min, z_max;
};

__device__ __forceinline__ exact::V3 nan3() {
  const float nan = __int_as_float(0x7FC00000);
  return {nan, nan, nan};
}

// the pixel's point; NaNs for an invalid pixel and for one outside the image
template <bool RAW16>
__device__ __forceinline__ exact::V3 load_point(const void* __restrict__ img, const unsigned char* __restrict__ mask, int u, int v,
                                                int rows, int cols, const Cam& c) {
  if (u < 0 || v < 0 || u >= rows || v >= cols) return nan3();
  const size_t i = (size_t)u * cols + v;
  const float d = depth_at<RAW16>(img, i);
  if (!((!mask || mask[i] != 0) && depth_ok(d, c.z_min, c.z_max))) return nan3();
  const float3 p = depth_point(u, v, d, c.fx, c.fy, c.cx, c.cy);
  return {p.x, p.y, p.z};
}

__device__ __forceinline__ bool is_nan(float f) { return f != f; }

// (tolerance * k)^2, float products
__device__ __forceinline__ float reach2(float tol, int k) {
  const float t = exact::mul(tol, (float)k);
  return exact::mul(t, t);
}
// both valid (a NaN fails) and ((dx dx + dy dy) + dz dz) <= t2
__device__ __forceinline__ bool reach(exact::V3 a, exact::V3 b, float t2) { return exact::sqnorm_lr(exact::vsub(a, b)) <= t2; }

__device__ __forceinline__ exact::V3 at3(const float* x, const float* y, const float* z, int o) { return {x[o], y[o], z[o]}; }

// m / sqrt(|m|^2) when |m|^2 > 0, else no normal (NaNs)
__device__ __forceinline__ exact::V3 unit_or_nan(exact::V3 m) {
  const float z = exact::sqnorm_lr(m);
  if (!(z > 0.f)) return nan3();
  const float n = exact::sqrt_rn(z);
  return {exact::fdiv(m.x, n), exact::fdiv(m.y, n), exact::fdiv(m.z, n)};
}

// the tangent along one image axis from the points `s` pixels ahead (a) and behind (b); false when neither is reachable
__device__ __forceinline__ bool tangent(exact::V3 p, exact::V3 a, exact::V3 b, float t2, exact::V3* t) {
  const bool ra = reach(p, a, t2), rb = reach(p, b, t2);
  *t = ra && rb ? exact::vsub(a, b) : ra ? exact::vsub(a, p) : exact::vsub(p, b);
  return ra || rb;
}

template <bool RAW16>
__global__ __launch_bounds__(kThreads) void dn_normals(const void* __restrict__ img, const unsigned char* __restrict__ mask,
                                                       int rows, int cols, Cam cam, float tol, int s, int w,
                                                       float4* __restrict__ normals) {
  extern __shared__ float s_mem[];
  const int H = s + w;
  const int PW = kTw + 2 * H, PH = kTh + 2 * H, NW = kTw + 2 * w, NH = kTh + 2 * w;
  float* px = s_mem;
  float* py = px + PW * PH;
  float* pz = py + PW * PH;
  float* rx = pz + PW * PH;
  float* ry = rx + NW * NH;
  float* rz = ry + NW * NH;
  const int u0 = blockIdx.y * kTh, v0 = blockIdx.x * kTw;
  for (int o = threadIdx.x; o < PW * PH; o += kThreads) {
    const int r = o / PW, c = o - r * PW;
    const exact::V3 p = load_point<RAW16>(img, mask, u0 - H + r, v0 - H + c, rows, cols, cam);
    px[o] = p.x;
    py[o] = p.y;
    pz[o] = p.z;
  }
  __syncthreads();
  // raw normals of the tile + w: pixel (r, c) of this region is point (r + s, c + s)
  const float t2s = reach2(tol, s);
  for (int o = threadIdx.x; o < NW * NH; o += kThreads) {
    const int r = o / NW, c = o - r * NW;
    const int q = (r + s) * PW + c + s;
    const exact::V3 p = at3(px, py, pz, q);
    exact::V3 h, g, n = nan3();
    const bool has_h = tangent(p, at3(px, py, pz, q + s), at3(px, py, pz, q - s), t2s, &h);
    const bool has_g = tangent(p, at3(px, py, pz, q + s * PW), at3(px, py, pz, q - s * PW), t2s, &g);
    if (has_h && has_g) n = unit_or_nan(exact::cross(g, h));
    rx[o] = n.x;
    ry[o] = n.y;
    rz[o] = n.z;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < kTw * kTh; o += kThreads) {
    const int r = o / kTw, c = o - r * kTw;
    const int u = u0 + r, v = v0 + c;
    if (u >= rows || v >= cols) continue;
    const int qp = (r + H) * PW + c + H, qn = (r + w) * NW + c + w;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!is_nan(rx[qn])) {
      const exact::V3 p = at3(px, py, pz, qp);
      exact::V3 acc = {0.f, 0.f, 0.f};
      for (int du = -w; du <= w; ++du)
        for (int dv = -w; dv <= w; ++dv) {
          const exact::V3 n = at3(rx, ry, rz, qn + du * NW + dv);
          bool on = du == 0 && dv == 0;
          if (!on) {
            const int k = max(abs(du), abs(dv));
            on = !is_nan(n.x) && reach(p, at3(px, py, pz, qp + du * PW + dv), reach2(tol, k));
          }
          if (on) acc = {exact::add(acc.x, n.x), exact::add(acc.y, n.y), exact::add(acc.z, n.z)};
        }
      const exact::V3 n = unit_or_nan(acc);
      if (!is_nan(n.x)) out = make_float4(n.x, n.y, n.z, 1.f);
    }
    normals[(size_t)u * cols + v] = out;
  }
}

template <bool RAW16>
__global__ __launch_bounds__(kThreads) void dn_crease(const void* __restrict__ img, const unsigned char* __restrict__ mask,
                                                      int rows, int cols, Cam cam, float tol, int c, float concavity,
                                                      const float4* __restrict__ normals, unsigned char* __restrict__ keep,
                                                      int* __restrict__ n_crease) {
  extern __shared__ float s_mem[];
  __shared__ int s_count[kThreads / 64];
  const int W = kTw + 2 * c, Hh = kTh + 2 * c;
  float* px = s_mem;
  float* py = px + W * Hh;
  float* pz = py + W * Hh;
  float* nx = pz + W * Hh;
  float* ny = nx + W * Hh;
  float* nz = ny + W * Hh;
  const int u0 = blockIdx.y * kTh, v0 = blockIdx.x * kTw;
  for (int o = threadIdx.x; o < W * Hh; o += kThreads) {
    const int r = o / W, q = o - r * W;
    const int u = u0 - c + r, v = v0 - c + q;
    const exact::V3 p = load_point<RAW16>(img, mask, u, v, rows, cols, cam);
    exact::V3 n = nan3();
    if (!is_nan(p.z)) {   // (valid, hence inside the image)
      const float4 f = normals[(size_t)u * cols + v];
      if (f.w != 0.f) n = {f.x, f.y, f.z};
    }
    px[o] = p.x;
    py[o] = p.y;
    pz[o] = p.z;
    nx[o] = n.x;
    ny[o] = n.y;
    nz[o] = n.z;
  }
  __syncthreads();
  const float t2 = reach2(tol, c);
  int creases = 0;
  for (int o = threadIdx.x; o < kTw * kTh; o += kThreads) {   // (workgroup-uniform trip count: the ballot below is whole)
    const int r = o / kTw, q = o - r * kTw;
    const int u = u0 + r, v = v0 + q;
    const bool inside = u < rows && v < cols;
    const int at = (r + c) * W + q + c;
    const exact::V3 pi = at3(px, py, pz, at), ni = at3(nx, ny, nz, at);
    bool crease = false;
    if (inside && !is_nan(ni.x)) {
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        if (e == 4) continue;
        const int off = (e / 3 - 1) * c * W + (e % 3 - 1) * c;
        const exact::V3 pj = at3(px, py, pz, at + off), nj = at3(nx, ny, nz, at + off);
        if (is_nan(nj.x) || !reach(pi, pj, t2)) continue;
        if (exact::dot_lr(exact::vsub(nj, ni), exact::vsub(pj, pi)) < 0.f)   // concave
          crease = crease || exact::sub(1.f, exact::dot_lr(ni, nj)) > concavity;
      }
    }
    if (inside) keep[(size_t)u * cols + v] = !is_nan(pi.z) && !crease ? 1 : 0;
    creases += __popcll(__ballot(crease));
  }
  wave::block4_publish(s_count, wave::lane() == 0, creases);
  if (threadIdx.x == 0) {   // one atomic per workgroup
    const int total = wave::block4_total(s_count);
    if (total) atomicAdd(n_crease, total);
  }
}

// one Jacobi pass: out = in, but a valid pixel with id 0 takes the smallest non-zero id of its reachable 4-neighbours
template <bool RAW16>
__global__ __launch_bounds__(kThreads) void dn_grow(const void* __restrict__ img, const unsigned char* __restrict__ mask,
                                                    int rows, int cols, Cam cam, float tol, const int* __restrict__ in,
                                                    int* __restrict__ out, int* __restrict__ n_grown) {
  __shared__ int s_count[kThreads / 64];
  const size_t n = (size_t)rows * cols;
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  bool grew = false;
  if (i < n) {
    int id = in[i];
    if (id == 0) {
      const int u = (int)(i / (size_t)cols), v = (int)(i - (size_t)u * cols);
      const exact::V3 p = load_point<RAW16>(img, mask, u, v, rows, cols, cam);
      if (!is_nan(p.z)) {
        const float t2 = reach2(tol, 1);
        int best = INT_MAX;
        const int du[4] = {-1, 1, 0, 0}, dv[4] = {0, 0, -1, 1};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int a = u + du[e], b = v + dv[e];
          if (a < 0 || b < 0 || a >= rows || b >= cols) continue;
          const int other = in[(size_t)a * cols + b];
          if (other != 0 && other < best && reach(p, load_point<RAW16>(img, mask, a, b, rows, cols, cam), t2)) best = other;
        }
        if (best != INT_MAX) {
          id = best;
          grew = true;
        }
      }
    }
    out[i] = id;
  }
  const int grown = __popcll(__ballot(grew));
  wave::block4_publish(s_count, wave::lane() == 0, grown);
  if (threadIdx.x == 0) {
    const int total = wave::block4_total(s_count);
    if (total) atomicAdd(n_grown, total);
  }
}

// counts[2] of the cores' labelling saw the keep bytes: the crease pixels are valid pixels too
__global__ void dn_counts(int* __restrict__ counts) { counts[2] += counts[3]; }

inline Cam cam_of(const pgp_components_options* opt, const float K[9]) { return Cam{K[0], K[4], K[2], K[5], opt->z_min, opt->z_max}; }
inline dim3 tiles_of(int rows, int cols) { return dim3((unsigned)((cols + kTw - 1) / kTw), (unsigned)((rows + kTh - 1) / kTh)); }

}  // namespace

int launch_depth_normals(const pgp_components_options* opt, const pgp_crease_options* co, const void* d_img, bool raw16,
                         const unsigned char* d_mask, int rows, int cols, const float K[9], float* d_normals, hipStream_t st) {
  if ((size_t)rows * cols == 0) return PGP_OK;
  const int s = co->normal_step, w = co->smooth_radius, H = s + w;
  const size_t lds = (size_t)3 * 4 * ((size_t)(kTw + 2 * H) * (kTh + 2 * H) + (size_t)(kTw + 2 * w) * (kTh + 2 * w));
  const Cam cam = cam_of(opt, K);
  float4* out = reinterpret_cast<float4*>(d_normals);
  if (raw16)
    hipLaunchKernelGGL(dn_normals<true>, tiles_of(rows, cols), dim3(kThreads), lds, st, d_img, d_mask, rows, cols, cam,
                       opt->tolerance, s, w, out);
  else
    hipLaunchKernelGGL(dn_normals<false>, tiles_of(rows, cols), dim3(kThreads), lds, st, d_img, d_mask, rows, cols, cam,
                       opt->tolerance, s, w, out);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

int launch_depth_crease(const pgp_components_options* opt, const pgp_crease_options* co, const void* d_img, bool raw16,
                        const unsigned char* d_mask, int rows, int cols, const float K[9], const float* d_normals,
                        unsigned char* d_keep, int* d_n_crease, hipStream_t st) {
  PGP_HIP(hipMemsetAsync(d_n_crease, 0, 4, st));
  if ((size_t)rows * cols == 0) return PGP_OK;
  const int c = co->crease_step;
  const size_t lds = (size_t)6 * 4 * (size_t)(kTw + 2 * c) * (kTh + 2 * c);
  const Cam cam = cam_of(opt, K);
  const float4* nrm = reinterpret_cast<const float4*>(d_normals);
  if (raw16)
    hipLaunchKernelGGL(dn_crease<true>, tiles_of(rows, cols), dim3(kThreads), lds, st, d_img, d_mask, rows, cols, cam,
                       opt->tolerance, c, co->concavity, nrm, d_keep, d_n_crease);
  else
    hipLaunchKernelGGL(dn_crease<false>, tiles_of(rows, cols), dim3(kThreads), lds, st, d_img, d_mask, rows, cols, cam,
                       opt->tolerance, c, co->concavity, nrm, d_keep, d_n_crease);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

// normals | keep bytes | two id images: the context's workspace of the three calls
namespace {
struct CreaseWs {
  Carve cv;
  Carve::Piece<float> normals;
  Carve::Piece<unsigned char> keep;
  Carve::Piece<int> ids_a, ids_b;
  CreaseWs(size_t n, bool with_ids) {
    normals = cv.add<float>(4 * n, 256);
    keep = cv.add<unsigned char>(n, 256);
    ids_a = cv.add<int>(with_ids ? n : 0, 256);
    ids_b = cv.add<int>(with_ids ? n : 0, 256);
    cv.pad(256);
  }
};
}  // namespace

int launch_depth_crease_mask(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* co, const void* d_img,
                             bool raw16, const unsigned char* d_mask, int rows, int cols, const float K[9],
                             unsigned char* d_keep, int* d_n_crease, hipStream_t st) {
  CreaseWs ws((size_t)rows * cols, false);
  int rc = ws.cv.ensure(ctx->d_crease_ws);
  if (rc != PGP_OK) return rc;
  float* normals = ws.cv.at(ws.normals);
  if ((rc = launch_depth_normals(opt, co, d_img, raw16, d_mask, rows, cols, K, normals, st)) != PGP_OK) return rc;
  return launch_depth_crease(opt, co, d_img, raw16, d_mask, rows, cols, K, normals, d_keep, d_n_crease, st);
}

int launch_depth_objects(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* co, const void* d_img,
                         bool raw16, const unsigned char* d_mask, int rows, int cols, const float K[9], int* d_roots, int* d_ids,
                         pgp_component_info* d_info, int cap, int* d_counts, hipStream_t st) {
  const size_t n = (size_t)rows * cols;
  PGP_HIP(hipMemsetAsync(d_counts, 0, 20, st));
  if (n == 0) return PGP_OK;
  CreaseWs ws(n, true);
  int rc = ws.cv.ensure(ctx->d_crease_ws);
  if (rc != PGP_OK) return rc;
  float* normals = ws.cv.at(ws.normals);
  unsigned char* keep = ws.cv.at(ws.keep);
  if ((rc = launch_depth_normals(opt, co, d_img, raw16, d_mask, rows, cols, K, normals, st)) != PGP_OK) return rc;
  if ((rc = launch_depth_crease(opt, co, d_img, raw16, d_mask, rows, cols, K, normals, keep, d_counts + 3, st)) != PGP_OK) return rc;
  // the cores: the existing labelling behind the keep bytes (it clears counts[0..2] itself)
  int* cur = ws.cv.at(ws.ids_a);
  int* other = ws.cv.at(ws.ids_b);
  if ((rc = launch_depth_components(ctx, opt, d_img, raw16, keep, rows, cols, K, d_roots, cur, d_info, cap, d_counts, st)) != PGP_OK)
    return rc;
  const Cam cam = cam_of(opt, K);
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
  for (int pass = 0; pass < co->grow_passes; ++pass) {
    int* out = pass + 1 == co->grow_passes && d_ids ? d_ids : other;   // the last pass writes the caller's image
    if (raw16)
      hipLaunchKernelGGL(dn_grow<true>, grid, dim3(kThreads), 0, st, d_img, d_mask, rows, cols, cam, opt->tolerance,
                         (const int*)cur, out, d_counts + 4);
    else
      hipLaunchKernelGGL(dn_grow<false>, grid, dim3(kThreads), 0, st, d_img, d_mask, rows, cols, cam, opt->tolerance,
                         (const int*)cur, out, d_counts + 4);
    other = cur;
    cur = out;
  }
  if (co->grow_passes == 0 && d_ids) PGP_HIP(hipMemcpyAsync(d_ids, cur, n * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(dn_counts, dim3(1), dim3(1), 0, st, d_counts);
  PGP_HIP(hipGetLastError());
  // the rows' pixels, boxes, depth ranges and sums describe the grown ids
  if (cap > 0 && co->grow_passes > 0)
    return launch_component_table(ctx, opt, d_img, raw16, rows, cols, K, cur, d_info, cap, d_counts, st);
  return PGP_OK;
}

}  // namespace pgp
