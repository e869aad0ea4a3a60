// csrc/components.hip -- object proposals on gfx950: connected components of a depth image with a 3-D distance test
// between neighbouring pixels (Euclidean clustering on the organised image, what PCL's
// OrganizedConnectedComponentSegmentation + EuclideanClusterComparator do), their table, ranking and the byte masks the
// segment front end reads; and the vote that puts each object's 2-D mask into a component.  The rules are those of
// include/pgp.h (pgp_depth_components, pgp_assign_masks_to_components).  The reference has no such step.
//
// Mapping.  A label is the smallest row-major pixel index of the component, so every link of the union-find goes from
// the larger index to the smaller one, parents only ever decrease, and the result does not depend on scheduling.
//   cc_tile     grid of kTw x kTh tiles, 256 threads: a wave owns kTh / 4 rows of 64 pixels.  The horizontal
//               connectivity of a row is ONE ballot; a pixel's run start comes from the zero bits below its lane.  The
//               points stay in LDS; the vertical (and diagonal) edges between runs are united in an LDS union-find
//               (atomicMin on parent words).  An edge whose end points are already joined through the lane to its left
//               is skipped, so a flat region costs one union per run pair, not one per pixel.  The tile's roots are written
//               as global indices.
//   cc_seam     the pixels on a tile's right and bottom borders (and, for the anti-diagonal, its left border) are united
//               with their neighbours in the next tile in global memory: find both roots, atomicMin the larger root's
//               parent to the smaller, continue from the value it returns.
//   cc_flatten  every pixel takes its root; valid pixels, components and pixels per root are counted (integer atomics,
//               one per distinct root of a wave).
//   cc_collect  every root that passes the size test appends its key (pixels << 32 | ~root) to a list whose bound is
//               rows * cols / min_pixels; rocPRIM sorts the padded list descending: pixels descending, root ascending.
//   cc_rank / cc_table / cc_finish   the first min(kept, cap) keys get ids and info rows; one pass over the pixels writes
//               ids and folds bounding box, depth range and the integer coordinate sums into the rows: a wave folds its
//               lanes per distinct id first, then one set of integer atomics -- in LDS for the 16 largest components
//               (per-workgroup parts that cc_finish folds), in global memory for the rest.
//   cc_retable_clear / cc_retable / cc_finish   the table once more, of ids that depth_crease.hip has grown past the
//               labelling's own (launch_component_table): cc_table's fold over given ids, the pixel counts with it.
// No kernel waits for another workgroup, there is no cooperative launch and no float atomic: every loop ends because
// parents only decrease.
//
// assign_votes / assign_reduce: the n_objects x (id bound + 1) histogram of (object, component id) and its per-object
// argmax (the lower id on ties).

#include "pgp_internal.h"
#include "wave.h"
#include "depth_pixel.h"

#include <algorithm>
#include <climits>

#include <rocprim/rocprim.hpp>

namespace pgp {

namespace {

constexpr int kThreads = 256;
constexpr int kTw = 64, kTh = 16;                 // tile: one wave across, four rows per wave
constexpr int kRowsPerWave = kTh / (kThreads / 64);

struct Cam {
  float fx, fy, cx, cy;
  double z_min, z_max;
};

// the pixel's point; false (and NaNs, which fail every distance test) for an invalid pixel
template <bool RAW16>
__device__ __forceinline__ bool load_point(const void* __restrict__ img, const unsigned char* __restrict__ mask, int u, int v,
                                           int cols, const Cam& c, float3* p) {
  const size_t i = (size_t)u * cols + v;
  const float d = depth_at<RAW16>(img, i);
  const bool ok = (!mask || mask[i] != 0) && depth_ok(d, c.z_min, c.z_max);
  const float nan = __int_as_float(0x7FC00000);
  *p = ok ? depth_point(u, v, d, c.fx, c.fy, c.cx, c.cy) : make_float3(nan, nan, nan);
  return ok;
}

__device__ __forceinline__ bool near(float3 a, float3 b, float tol2) {
  const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)) <= tol2;
}

// ---- union-find: links go from the larger index to the smaller, so a root is the smallest index of its tree ----------
__device__ __forceinline__ int find_lds(volatile int* p, int a) {
  int q;
  while ((q = p[a]) != a) a = q;
  return a;
}

__device__ __forceinline__ void unite_lds(int* p, int a, int b) {
  for (;;) {
    a = find_lds(p, a);
    b = find_lds(p, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&p[a], b);
    if (old == a) return;
    a = old;   // a had been linked meanwhile: its former parent and b are still to be joined
  }
}

__device__ __forceinline__ int find_global(const int* p, int a) {
  int q;
  while ((q = __hip_atomic_load(&p[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a) a = q;
  return a;
}

__device__ __forceinline__ void unite_global(int* p, int a, int b) {
  for (;;) {
    a = find_global(p, a);
    b = find_global(p, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&p[a], b);
    if (old == a) return;
    a = old;
  }
}

template <bool RAW16>
__global__ __launch_bounds__(kThreads) void cc_tile(const void* __restrict__ img, const unsigned char* __restrict__ mask,
                                                    int rows, int cols, Cam cam, float tol2, int conn8,
                                                    int* __restrict__ parent) {
  __shared__ float s_x[kTh * kTw], s_y[kTh * kTw], s_z[kTh * kTw];
  __shared__ int s_par[kTh * kTw];
  __shared__ unsigned long long s_right[kTh];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.y * kTh, v0 = blockIdx.x * kTw;
  const int v = v0 + lane;
  bool valid[kRowsPerWave];
  // rows: points into LDS, runs from one ballot
#pragma unroll
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int r = wave * kRowsPerWave + k, u = u0 + r;
    const float nan = __int_as_float(0x7FC00000);
    float3 p = make_float3(nan, nan, nan);
    valid[k] = u < rows && v < cols && load_point<RAW16>(img, mask, u, v, cols, cam, &p);
    const float3 q = make_float3(__shfl_down(p.x, 1, 64), __shfl_down(p.y, 1, 64), __shfl_down(p.z, 1, 64));
    const unsigned long long right = __ballot(lane < 63 && near(p, q, tol2));   // bit l: lanes l and l + 1 are joined
    const unsigned long long gaps = ~right & ((1ull << lane) - 1ull);           // the breaks below this lane
    const int start = gaps ? 64 - __clzll(gaps) : 0;
    const int o = r * kTw + lane;
    s_x[o] = p.x;
    s_y[o] = p.y;
    s_z[o] = p.z;
    s_par[o] = valid[k] ? r * kTw + start : -1;
    if (lane == 0) s_right[r] = right;
  }
  __syncthreads();
  // the edges to the next row
#pragma unroll
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int r = wave * kRowsPerWave + k;
    if (r + 1 >= kTh) break;   // (wave-uniform) the tile's last row: cc_seam
    const int o = r * kTw + lane, ob = o + kTw;
    const float3 p = make_float3(s_x[o], s_y[o], s_z[o]);
    const unsigned long long here = s_right[r], below = s_right[r + 1];
    const bool down = near(p, make_float3(s_x[ob], s_y[ob], s_z[ob]), tol2);
    const unsigned long long dmask = __ballot(down);
    const bool left_here = lane > 0 && ((here >> (lane - 1)) & 1), left_below = lane > 0 && ((below >> (lane - 1)) & 1);
    const bool left_down = lane > 0 && ((dmask >> (lane - 1)) & 1);
    if (down && !(left_here && left_below && left_down)) unite_lds(s_par, o, ob);
    if (conn8) {
      if (lane < 63 && near(p, make_float3(s_x[ob + 1], s_y[ob + 1], s_z[ob + 1]), tol2)) {
        const bool via_down = down && ((below >> lane) & 1);
        const bool via_right = ((here >> lane) & 1) && ((dmask >> (lane + 1)) & 1);
        if (!via_down && !via_right) unite_lds(s_par, o, ob + 1);
      }
      if (lane > 0 && near(p, make_float3(s_x[ob - 1], s_y[ob - 1], s_z[ob - 1]), tol2)) {
        const bool via_down = down && left_below;
        const bool via_left = left_here && left_down;
        if (!via_down && !via_left) unite_lds(s_par, o, ob - 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRowsPerWave; ++k) {
    if (!valid[k]) continue;
    const int r = wave * kRowsPerWave + k;
    const int root = find_lds(s_par, r * kTw + lane);
    parent[(size_t)(u0 + r) * cols + v] = (u0 + root / kTw) * cols + v0 + root % kTw;
  }
}

// one thread per pixel; only the pixels of a tile's right, bottom (and, for the anti-diagonal, left) border go on
template <bool RAW16>
__global__ __launch_bounds__(kThreads) void cc_seam(const void* __restrict__ img, const unsigned char* __restrict__ mask,
                                                    int rows, int cols, Cam cam, float tol2, int conn8,
                                                    int* __restrict__ parent) {
  const size_t n = (size_t)rows * cols;
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int u = (int)(i / (size_t)cols), v = (int)(i - (size_t)u * cols);
  const bool has_r = v + 1 < cols, has_d = u + 1 < rows, has_l = v > 0;
  const bool on_right = (v % kTw) == kTw - 1 && has_r, on_bottom = (u % kTh) == kTh - 1 && has_d;
  const bool on_left = conn8 && (v % kTw) == 0 && has_l && has_d;
  if (!on_right && !on_bottom && !on_left) return;
  float3 p, q;
  if (!load_point<RAW16>(img, mask, u, v, cols, cam, &p)) return;
  if (on_right && load_point<RAW16>(img, mask, u, v + 1, cols, cam, &q) && near(p, q, tol2))
    unite_global(parent, (int)i, (int)i + 1);
  if (on_bottom && load_point<RAW16>(img, mask, u + 1, v, cols, cam, &q) && near(p, q, tol2))
    unite_global(parent, (int)i, (int)i + cols);
  if (!conn8) return;
  if ((on_right || on_bottom) && has_r && has_d && load_point<RAW16>(img, mask, u + 1, v + 1, cols, cam, &q) && near(p, q, tol2))
    unite_global(parent, (int)i, (int)i + cols + 1);
  if ((on_left || on_bottom) && has_l && has_d && load_point<RAW16>(img, mask, u + 1, v - 1, cols, cam, &q) && near(p, q, tol2))
    unite_global(parent, (int)i, (int)i + cols - 1);
}

// counts[1] components, counts[2] valid pixels; pixels[root] the size of each component
__global__ __launch_bounds__(kThreads) void cc_flatten(const int* __restrict__ parent, size_t n, int* __restrict__ roots,
                                                       int* __restrict__ pixels, int* __restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  __shared__ int s_valid[kThreads / 64], s_heads[kThreads / 64];
  const int lane = threadIdx.x & 63;
  int root = -1;
  if (i < n && parent[i] >= 0) root = find_global(parent, parent[i]);
  if (i < n) roots[i] = root;
  const bool valid = root >= 0;
  unsigned long long todo = __ballot(valid);
  const unsigned long long heads = __ballot(valid && (size_t)root == i);
  if (lane == 0) {
    s_valid[threadIdx.x >> 6] = __popcll(todo);
    s_heads[threadIdx.x >> 6] = __popcll(heads);
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // one pair of atomics per workgroup
    const int nv = wave::block4_total(s_valid), nh = wave::block4_total(s_heads);
    if (nv) atomicAdd(&counts[2], nv);
    if (nh) atomicAdd(&counts[1], nh);
  }
  while (todo) {   // (wave-uniform) one atomic per distinct root of the wave
    const int leader = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(root, leader, 64);
    const unsigned long long same = __ballot(valid && root == r0);
    if (lane == leader) atomicAdd(&pixels[r0], __popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(kThreads) void cc_collect(const int* __restrict__ roots, const int* __restrict__ pixels,
                                                       size_t n, int min_pixels, int max_pixels,
                                                       unsigned long long* __restrict__ keys, size_t key_cap,
                                                       int* __restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n || (size_t)roots[i] != i || roots[i] < 0) return;
  const int c = pixels[i];
  if (c < min_pixels || (max_pixels > 0 && c > max_pixels)) return;
  const size_t slot = (size_t)atomicAdd(&counts[0], 1);
  if (slot < key_cap)   // (always: a kept component has at least min_pixels pixels)
    keys[slot] = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}

// order-preserving image of a float in unsigned integers (-0 below +0)
__device__ __forceinline__ unsigned ordered_bits(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the neutral row of the table's folds (the depth range as ordered bits until cc_finish)
__device__ __forceinline__ void row_clear(pgp_component_info* r) {
  r->u_min = r->v_min = INT_MAX;
  r->u_max = r->v_max = INT_MIN;
  r->z_min = __uint_as_float(0xFFFFFFFFu);
  r->z_max = __uint_as_float(0u);
  r->sum_um[0] = r->sum_um[1] = r->sum_um[2] = 0;
}

// sorted key k -> id k + 1: pixels[root] = -(k + 1) (what cc_table reads), and the info row's starting values
__global__ __launch_bounds__(kThreads) void cc_rank(const unsigned long long* __restrict__ keys, const int* __restrict__ counts,
                                                    int cap, int* __restrict__ pixels, pgp_component_info* __restrict__ info) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= cap || k >= counts[0]) return;
  const unsigned long long key = keys[k];
  const int root = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
  pixels[root] = -(k + 1);
  pgp_component_info r;
  r.root = root;
  r.pixels = (int)(key >> 32);
  row_clear(&r);
  info[k] = r;
}

// integer atomics on one row, in LDS or in global memory
__device__ __forceinline__ void row_fold(pgp_component_info* r, int u_lo, int u_hi, int v_lo, int v_hi, unsigned z_lo,
                                         unsigned z_hi, const long long t[3]) {
  atomicMin(&r->u_min, u_lo);
  atomicMax(&r->u_max, u_hi);
  atomicMin(&r->v_min, v_lo);
  atomicMax(&r->v_max, v_hi);
  atomicMin(reinterpret_cast<unsigned*>(&r->z_min), z_lo);
  atomicMax(reinterpret_cast<unsigned*>(&r->z_max), z_hi);
#pragma unroll
  for (int k = 0; k < 3; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_um[k]), (unsigned long long)t[k]);
}

// ids, and the table.  A workgroup walks 256-pixel chunks; a wave folds its lanes per distinct id, then its first lane of
// that id adds the fold to the row.  The rows of the first kLdsIds ids -- the largest components, where every wave of the
// image would otherwise queue on the same few words of the L2 -- are kept per workgroup in LDS and leave as plain stores
// to part[workgroup][id - 1], which cc_finish folds; the other ids go to their info rows with global atomics.
constexpr int kLdsIds = 16;
constexpr int kTableBlocks = 256;

template <bool RAW16>
__global__ __launch_bounds__(kThreads) void cc_table(const void* __restrict__ img, int cols, Cam cam,
                                                     const int* __restrict__ roots, const int* __restrict__ pixels, size_t n,
                                                     int* __restrict__ ids, pgp_component_info* __restrict__ info,
                                                     pgp_component_info* __restrict__ part) {
  __shared__ pgp_component_info s_row[kLdsIds];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < kLdsIds) row_clear(&s_row[threadIdx.x]);
  __syncthreads();
  const size_t n_chunks = (n + kThreads - 1) / kThreads;
  for (size_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {   // (workgroup-uniform)
    const size_t i = ch * kThreads + threadIdx.x;
    int id = 0;
    if (i < n) {
      const int root = roots[i];
      if (root >= 0) {
        const int c = pixels[root];
        id = c < 0 ? -c : 0;
      }
      if (ids) ids[i] = id;
    }
    if (!info) continue;   // (uniform)
    int u = 0, v = 0;
    unsigned zk = 0;
    long long s[3] = {0, 0, 0};
    if (id > 0) {
      u = (int)(i / (size_t)cols);
      v = (int)(i - (size_t)u * cols);
      const float3 p = depth_point(u, v, depth_at<RAW16>(img, i), cam.fx, cam.fy, cam.cx, cam.cy);
      zk = ordered_bits(p.z);
      s[0] = llrint((double)p.x * 1e6);
      s[1] = llrint((double)p.y * 1e6);
      s[2] = llrint((double)p.z * 1e6);
    }
    unsigned long long todo = __ballot(id > 0);
    while (todo) {   // (wave-uniform)
      const int leader = __ffsll((long long)todo) - 1;
      const int id0 = __shfl(id, leader, 64);
      const bool in = id == id0;
      todo &= ~__ballot(in);
      const int u_lo = wave::min(in ? u : INT_MAX), u_hi = wave::max(in ? u : INT_MIN);
      const int v_lo = wave::min(in ? v : INT_MAX), v_hi = wave::max(in ? v : INT_MIN);
      const unsigned z_lo = wave::min(in ? zk : 0xFFFFFFFFu), z_hi = wave::max(in ? zk : 0u);
      long long t[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = wave::sum(in ? s[k] : 0ll);
      if (lane == leader) {
        if (id0 <= kLdsIds) row_fold(&s_row[id0 - 1], u_lo, u_hi, v_lo, v_hi, z_lo, z_hi, t);
        else row_fold(info + (id0 - 1), u_lo, u_hi, v_lo, v_hi, z_lo, z_hi, t);
      }
    }
  }
  if (!info) return;
  __syncthreads();
  if (threadIdx.x < kLdsIds) part[(size_t)blockIdx.x * kLdsIds + threadIdx.x] = s_row[threadIdx.x];
}

// one wave per written row: the first kLdsIds rows fold their per-workgroup parts, every row's depth range becomes floats
__global__ __launch_bounds__(64) void cc_finish(const int* __restrict__ counts, int cap, pgp_component_info* __restrict__ info,
                                                const pgp_component_info* __restrict__ part, int n_parts) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= cap || k >= counts[0]) return;
  pgp_component_info r = info[k];
  if (k < kLdsIds) {
    row_clear(&r);
    for (int b = lane; b < n_parts; b += 64) {
      const pgp_component_info q = part[(size_t)b * kLdsIds + k];
      r.u_min = min(r.u_min, q.u_min);
      r.u_max = max(r.u_max, q.u_max);
      r.v_min = min(r.v_min, q.v_min);
      r.v_max = max(r.v_max, q.v_max);
      r.z_min = __uint_as_float(min(__float_as_uint(r.z_min), __float_as_uint(q.z_min)));
      r.z_max = __uint_as_float(max(__float_as_uint(r.z_max), __float_as_uint(q.z_max)));
      for (int c = 0; c < 3; ++c) r.sum_um[c] += q.sum_um[c];
    }
    r.u_min = wave::min(r.u_min);
    r.u_max = wave::max(r.u_max);
    r.v_min = wave::min(r.v_min);
    r.v_max = wave::max(r.v_max);
    r.z_min = __uint_as_float(wave::min(__float_as_uint(r.z_min)));
    r.z_max = __uint_as_float(wave::max(__float_as_uint(r.z_max)));
    for (int c = 0; c < 3; ++c) r.sum_um[c] = wave::sum(r.sum_um[c]);
  }
  if (lane != 0) return;
  info[k].u_min = r.u_min;
  info[k].u_max = r.u_max;
  info[k].v_min = r.v_min;
  info[k].v_max = r.v_max;
  info[k].z_min = ordered_float(__float_as_uint(r.z_min));
  info[k].z_max = ordered_float(__float_as_uint(r.z_max));
  for (int c = 0; c < 3; ++c) info[k].sum_um[c] = r.sum_um[c];
}

__global__ __launch_bounds__(kThreads) void cc_mask(const int* __restrict__ ids, size_t n, int id, unsigned char* __restrict__ mask) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) mask[i] = ids[i] == id ? 1 : 0;
}

// ---- masks -> components -------------------------------------------------------------------------------------------
struct ClassValues {
  int v[kAssignMaxObjects];
};

template <class T>
__global__ __launch_bounds__(kThreads) void assign_votes(const int* __restrict__ ids, const T* __restrict__ classes, size_t n,
                                                         ClassValues cv, int n_obj, int id_bound, int* __restrict__ hist,
                                                         int* __restrict__ flag) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int id = 0, cls = -1;
  if (i < n) {
    id = ids[i];
    cls = (int)classes[i];
    if (id < 0 || id > id_bound) {
      atomicOr(flag, 1);
      id = 0;
    }
  }
  if (!__ballot(id != 0)) return;
  for (int o = 0; o < n_obj; ++o) {   // (uniform) one atomic per (object, distinct id of the wave)
    const bool hit = id != 0 && cls == cv.v[o];
    unsigned long long todo = __ballot(hit);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int id0 = __shfl(id, leader, 64);
      const unsigned long long same = __ballot(hit && id == id0);
      if (lane == leader) atomicAdd(&hist[(size_t)o * (id_bound + 1) + id0], __popcll(same));
      todo &= ~same;
    }
  }
}

// one workgroup per object: the total and the fullest column of its row, the lower id on ties
__global__ __launch_bounds__(kThreads) void assign_reduce(const int* __restrict__ hist, int id_bound, const int* __restrict__ flag,
                                                          int* __restrict__ result, int n_obj) {
  __shared__ int s_best[kThreads], s_id[kThreads], s_tot[kThreads];
  const int o = blockIdx.x, t = threadIdx.x;
  const int* row = hist + (size_t)o * (id_bound + 1);
  int best = 0, bid = 0, tot = 0;
  for (int k = 1 + t; k <= id_bound; k += kThreads) {   // ascending ids per thread: strict > keeps the lower one
    const int c = row[k];
    tot += c;
    if (c > best) {
      best = c;
      bid = k;
    }
  }
  s_best[t] = best;
  s_id[t] = bid;
  s_tot[t] = tot;
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if (t < off) {
      const int b = s_best[t + off], d = s_id[t + off];
      if (b > s_best[t] || (b == s_best[t] && b > 0 && d < s_id[t])) {
        s_best[t] = b;
        s_id[t] = d;
      }
      s_tot[t] += s_tot[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    result[3 * o] = s_tot[0] > 0 ? s_id[0] : 0;
    result[3 * o + 1] = s_best[0];
    result[3 * o + 2] = s_tot[0];
    if (o == 0) result[3 * n_obj] = *flag;
  }
}

inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace

int launch_depth_components(pgp_ctx* ctx, const pgp_components_options* opt, const void* d_img, bool raw16,
                            const unsigned char* d_mask, int rows, int cols, const float K[9], int* d_roots, int* d_ids,
                            pgp_component_info* d_info, int cap, int* d_counts, hipStream_t st) {
  const size_t n = (size_t)rows * cols;
  PGP_HIP(hipMemsetAsync(d_counts, 0, 12, st));
  if (n == 0) return PGP_OK;
  const size_t key_cap = n / (size_t)opt->min_pixels;   // a kept component has at least min_pixels pixels
  size_t sort_bytes = 0;
  if (key_cap > 0) {
    const hipError_t he = rocprim::radix_sort_keys_desc(nullptr, sort_bytes, (unsigned long long*)nullptr,
                                                        (unsigned long long*)nullptr, key_cap, 0, 64, st);
    if (he != hipSuccess) {
      set_error("rocprim::radix_sort_keys_desc (size query) failed: %s", hipGetErrorString(he));
      return PGP_EHIP;
    }
  }
  Carve cv;
  const auto c_parent = cv.add<int>(n, 256), c_roots = cv.add<int>(d_roots ? 0 : n, 256), c_pixels = cv.add<int>(n, 256);
  const auto c_keys = cv.add<unsigned long long>(2 * key_cap, 256);
  const auto c_sort = cv.add<unsigned char>(sort_bytes, 256);
  const int table_blocks = (int)std::min<size_t>((n + kThreads - 1) / kThreads, (size_t)kTableBlocks);
  const auto c_part = cv.add<pgp_component_info>((size_t)table_blocks * kLdsIds, 256);
  cv.pad(256);
  int rc = cv.ensure(ctx->d_cc_ws);
  if (rc != PGP_OK) return rc;
  int* parent = cv.at(c_parent);
  int* roots = d_roots ? d_roots : cv.at(c_roots);
  int* pixels = cv.at(c_pixels);
  unsigned long long* keys = cv.at(c_keys);
  unsigned long long* sorted = keys + key_cap;
  const Cam cam{K[0], K[4], K[2], K[5], opt->z_min, opt->z_max};
  const float tol2 = opt->tolerance * opt->tolerance;
  const int conn8 = opt->connectivity == 8;
  PGP_HIP(hipMemsetAsync(parent, 0xFF, n * 4, st));   // -1: invalid until cc_tile says otherwise
  PGP_HIP(hipMemsetAsync(pixels, 0, n * 4, st));
  if (key_cap > 0) PGP_HIP(hipMemsetAsync(keys, 0, key_cap * 8, st));   // padding sorts last
  const dim3 tiles((unsigned)((cols + kTw - 1) / kTw), (unsigned)((rows + kTh - 1) / kTh));
  if (raw16) {
    hipLaunchKernelGGL(cc_tile<true>, tiles, dim3(kThreads), 0, st, d_img, d_mask, rows, cols, cam, tol2, conn8, parent);
    hipLaunchKernelGGL(cc_seam<true>, grid_for(n), dim3(kThreads), 0, st, d_img, d_mask, rows, cols, cam, tol2, conn8, parent);
  } else {
    hipLaunchKernelGGL(cc_tile<false>, tiles, dim3(kThreads), 0, st, d_img, d_mask, rows, cols, cam, tol2, conn8, parent);
    hipLaunchKernelGGL(cc_seam<false>, grid_for(n), dim3(kThreads), 0, st, d_img, d_mask, rows, cols, cam, tol2, conn8, parent);
  }
  hipLaunchKernelGGL(cc_flatten, grid_for(n), dim3(kThreads), 0, st, (const int*)parent, n, roots, pixels, d_counts);
  hipLaunchKernelGGL(cc_collect, grid_for(n), dim3(kThreads), 0, st, (const int*)roots, (const int*)pixels, n, opt->min_pixels,
                     opt->max_pixels, keys, key_cap, d_counts);
  const int n_rank = (int)(key_cap < (size_t)cap ? key_cap : (size_t)cap);   // ids handed out at most
  if (n_rank > 0) {
    const hipError_t he = rocprim::radix_sort_keys_desc(cv.at(c_sort), sort_bytes, keys, sorted, key_cap, 0, 64, st);
    if (he != hipSuccess) {
      set_error("rocprim::radix_sort_keys_desc failed: %s", hipGetErrorString(he));
      return PGP_EHIP;
    }
    hipLaunchKernelGGL(cc_rank, grid_for((size_t)n_rank), dim3(kThreads), 0, st, (const unsigned long long*)sorted,
                       (const int*)d_counts, n_rank, pixels, d_info);
  }
  if (d_ids || n_rank > 0) {
    pgp_component_info* info = n_rank > 0 ? d_info : nullptr;
    if (raw16)
      hipLaunchKernelGGL(cc_table<true>, dim3(table_blocks), dim3(kThreads), 0, st, d_img, cols, cam, (const int*)roots,
                         (const int*)pixels, n, d_ids, info, cv.at(c_part));
    else
      hipLaunchKernelGGL(cc_table<false>, dim3(table_blocks), dim3(kThreads), 0, st, d_img, cols, cam, (const int*)roots,
                         (const int*)pixels, n, d_ids, info, cv.at(c_part));
  }
  if (n_rank > 0)
    hipLaunchKernelGGL(cc_finish, dim3(n_rank), dim3(64), 0, st, (const int*)d_counts, n_rank, d_info,
                       (const pgp_component_info*)cv.at(c_part), table_blocks);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

// ---- the table of an id image that is no longer the labelling's own (depth_crease.hip: the grown ids) ---------------
namespace {

// rows 0 .. min(kept, cap) - 1 keep their root; pixels and the folds start again
__global__ __launch_bounds__(kThreads) void cc_retable_clear(const int* __restrict__ counts, int cap,
                                                             pgp_component_info* __restrict__ info) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= cap || k >= counts[0]) return;
  info[k].pixels = 0;
  row_clear(&info[k]);
}

// cc_table's fold over given ids (values 0 .. min(kept, cap)); the pixel counts, which cc_table takes from the sort keys,
// are one integer atomic per wave and distinct id on the row itself
template <bool RAW16>
__global__ __launch_bounds__(kThreads) void cc_retable(const void* __restrict__ img, int cols, Cam cam, const int* __restrict__ ids,
                                                       size_t n, pgp_component_info* __restrict__ info,
                                                       pgp_component_info* __restrict__ part) {
  __shared__ pgp_component_info s_row[kLdsIds];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < kLdsIds) row_clear(&s_row[threadIdx.x]);
  __syncthreads();
  const size_t n_chunks = (n + kThreads - 1) / kThreads;
  for (size_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {   // (workgroup-uniform)
    const size_t i = ch * kThreads + threadIdx.x;
    const int id = i < n ? ids[i] : 0;
    int u = 0, v = 0;
    unsigned zk = 0;
    long long s[3] = {0, 0, 0};
    if (id > 0) {
      u = (int)(i / (size_t)cols);
      v = (int)(i - (size_t)u * cols);
      const float3 p = depth_point(u, v, depth_at<RAW16>(img, i), cam.fx, cam.fy, cam.cx, cam.cy);
      zk = ordered_bits(p.z);
      s[0] = llrint((double)p.x * 1e6);
      s[1] = llrint((double)p.y * 1e6);
      s[2] = llrint((double)p.z * 1e6);
    }
    unsigned long long todo = __ballot(id > 0);
    while (todo) {   // (wave-uniform)
      const int leader = __ffsll((long long)todo) - 1;
      const int id0 = __shfl(id, leader, 64);
      const bool in = id == id0;
      const unsigned long long same = __ballot(in);
      todo &= ~same;
      const int u_lo = wave::min(in ? u : INT_MAX), u_hi = wave::max(in ? u : INT_MIN);
      const int v_lo = wave::min(in ? v : INT_MAX), v_hi = wave::max(in ? v : INT_MIN);
      const unsigned z_lo = wave::min(in ? zk : 0xFFFFFFFFu), z_hi = wave::max(in ? zk : 0u);
      long long t[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = wave::sum(in ? s[k] : 0ll);
      if (lane == leader) {
        atomicAdd(&info[id0 - 1].pixels, __popcll(same));
        if (id0 <= kLdsIds) row_fold(&s_row[id0 - 1], u_lo, u_hi, v_lo, v_hi, z_lo, z_hi, t);
        else row_fold(info + (id0 - 1), u_lo, u_hi, v_lo, v_hi, z_lo, z_hi, t);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kLdsIds) part[(size_t)blockIdx.x * kLdsIds + threadIdx.x] = s_row[threadIdx.x];
}

}  // namespace

// d_ids: the ids of the launch_depth_components call just queued on `st` with the same options, shape and cap, regrown by
// the caller (a pixel with id 0 may have taken an id; no id has lost a pixel).  Rewrites pixels, box, depth range and sums
// of its info rows; their order and roots stay.
int launch_component_table(pgp_ctx* ctx, const pgp_components_options* opt, const void* d_img, bool raw16, int rows, int cols,
                           const float K[9], const int* d_ids, pgp_component_info* d_info, int cap, const int* d_counts,
                           hipStream_t st) {
  const size_t n = (size_t)rows * cols;
  const size_t key_cap = n / (size_t)opt->min_pixels;
  const int n_rank = (int)(key_cap < (size_t)cap ? key_cap : (size_t)cap);
  if (n_rank <= 0) return PGP_OK;
  const int table_blocks = (int)std::min<size_t>((n + kThreads - 1) / kThreads, (size_t)kTableBlocks);
  Carve cv;
  const auto c_part = cv.add<pgp_component_info>((size_t)table_blocks * kLdsIds, 256);
  cv.pad(256);
  // (the labelling's workspace: free once its results are out, calls on one context are ordered, and that call sized it
  //  for these parts among the rest, so nothing is allocated here)
  int rc = cv.ensure(ctx->d_cc_ws);
  if (rc != PGP_OK) return rc;
  const Cam cam{K[0], K[4], K[2], K[5], opt->z_min, opt->z_max};
  hipLaunchKernelGGL(cc_retable_clear, grid_for((size_t)n_rank), dim3(kThreads), 0, st, d_counts, n_rank, d_info);
  if (raw16)
    hipLaunchKernelGGL(cc_retable<true>, dim3(table_blocks), dim3(kThreads), 0, st, d_img, cols, cam, d_ids, n, d_info,
                       cv.at(c_part));
  else
    hipLaunchKernelGGL(cc_retable<false>, dim3(table_blocks), dim3(kThreads), 0, st, d_img, cols, cam, d_ids, n, d_info,
                       cv.at(c_part));
  hipLaunchKernelGGL(cc_finish, dim3(n_rank), dim3(64), 0, st, d_counts, n_rank, d_info,
                     (const pgp_component_info*)cv.at(c_part), table_blocks);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

int launch_component_mask(const int* d_ids, size_t n, int id, unsigned char* d_mask, hipStream_t st) {
  if (n == 0) return PGP_OK;
  hipLaunchKernelGGL(cc_mask, grid_for(n), dim3(kThreads), 0, st, d_ids, n, id, d_mask);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

int launch_assign_masks(pgp_ctx* ctx, const int* d_ids, const void* d_classes, int class_bytes, size_t n,
                        const int* class_values, int n_objects, int* d_result, hipStream_t st) {
  const int id_bound = (int)(n < (size_t)kAssignMaxId ? n : (size_t)kAssignMaxId);   // an id names a component of >= 1 pixel
  Carve cv;
  const auto c_hist = cv.add<int>((size_t)n_objects * (id_bound + 1), 256), c_flag = cv.add<int>(1, 256);
  cv.pad(256);
  // (the labelling's workspace: free once its results are out, and calls on one context are ordered)
  int rc = cv.ensure(ctx->d_cc_ws);
  if (rc != PGP_OK) return rc;
  int* hist = cv.at(c_hist);
  int* flag = cv.at(c_flag);
  PGP_HIP(hipMemsetAsync(hist, 0, cv.bytes(), st));   // the flag with it
  ClassValues vals;
  for (int o = 0; o < kAssignMaxObjects; ++o) vals.v[o] = o < n_objects ? class_values[o] : 0;
  if (n > 0) {
    if (class_bytes == 1)
      hipLaunchKernelGGL(assign_votes<unsigned char>, grid_for(n), dim3(kThreads), 0, st, d_ids,
                         static_cast<const unsigned char*>(d_classes), n, vals, n_objects, id_bound, hist, flag);
    else
      hipLaunchKernelGGL(assign_votes<unsigned short>, grid_for(n), dim3(kThreads), 0, st, d_ids,
                         static_cast<const unsigned short*>(d_classes), n, vals, n_objects, id_bound, hist, flag);
  }
  hipLaunchKernelGGL(assign_reduce, dim3(n_objects), dim3(kThreads), 0, st, (const int*)hist, id_bound, (const int*)flag, d_result,
                     n_objects);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

}  // namespace pgp
