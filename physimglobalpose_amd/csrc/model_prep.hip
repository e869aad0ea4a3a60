// csrc/model_prep.hip -- a new object's model clouds from its mesh: area-weighted surface sampling with face normals, and
// the farthest-point order of a cloud (every prefix of the order is a well-spread subset: one ordered validation cloud
// also holds the search cloud as its first rows).  The node reads both clouds from files prepared offline
// (PPE/data_layer/Objects.cpp:22-28) and ships no tool that writes them.  Both rules are stated in include/pgp.h and
// restated in numpy by tests/_model_prep_restate.py; every output is reproduced bit for bit.
//
// SAMPLING.  Triangle areas in double (every operation rounded on its own), their exact maximum by a 64-bit atomic max on
// the bit pattern (a non-negative double orders as its bits do), INTEGER weights w = floor(A / A_max 2^32) so that no
// summation order shows, their inclusive prefix sums C in uint64 (rocPRIM; integer addition is exact under any tree),
// then one thread per sample: four 31-bit variates of its own counter-based stream, a 62-bit fraction of W = C[last], a
// binary search of C, the point by two lerps and the face normal through exact::.  A bad index or a non-finite vertex
// raises a flag and gives its triangle the area 0, so that nothing is read out of bounds before the host has seen the
// flag; W == 0 writes nothing.
//
// FARTHEST POINTS.  Every point keeps d = the smallest squared distance to a picked point (-1 once picked); the next pick
// is the largest d, ties to the lowest index.  The arg-max is a max over 64-bit keys: d's bit pattern (d >= 0) high,
// ~index low, 0 for a picked point.
//   resident form (n <= 16384): ONE workgroup of 1024 threads; thread t keeps the points t + 1024 j and their d in
//     registers for all k picks.  Per pick: update + local arg-max, a shuffle max over the wave, the wave's record {key,
//     the winner's coordinates} into one of two LDS banks, ONE __syncthreads(), every lane reads the 16 records.
//     (Two banks: a wave that runs ahead into pick j + 1 writes the other bank; it reaches pick j + 2's write only behind
//      pick j + 1's barrier, by which every lane has read pick j's records.)
//   multi-launch form (larger n; PGP_FPS_FORM=multi at any n): one launch per pick over G <= 256 workgroups, each owning
//     the slice [g L, (g + 1) L).  Every workgroup max-reduces the G partial keys the launch before it left (= the pick;
//     workgroup 0 records it), updates its slice of d in HBM and leaves its own partial key in the OTHER of two partial
//     arrays.  The k launches are queued back to back; no workgroup waits for another inside a kernel.

#include <cstring>  // rocprim's texture_cache_iterator.hpp uses memset without including it

#include "exact_f32.h"
#include "pgp_internal.h"
#include "wave.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cfloat>
#include <cstdlib>

namespace pgp {

using exact::V3;

namespace {

// ---------------------------------------------------------------------------------------------------------- sampling

struct SampleMeta {
  unsigned long long amax_bits;   // bit pattern of the largest area
  unsigned int err;               // kErr* bits
  unsigned int pad;
};
constexpr unsigned int kErrIndex = 1u, kErrVertex = 2u;

__device__ __forceinline__ V3 vertex_at(const float* __restrict__ v, int stride, int i) {
  const float* p = v + (size_t)stride * (size_t)i;
  return {p[0], p[1], p[2]};
}

// thread i: the area of triangle i (i < n_tri) and the finiteness of vertex i (i < n_vert)
__global__ __launch_bounds__(256) void prep_areas(const float* __restrict__ vert, int n_vert, int stride,
                                                  const int* __restrict__ tri, int n_tri, double* __restrict__ area,
                                                  SampleMeta* meta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned int err = 0u;
  if (i < n_vert) {
    const V3 p = vertex_at(vert, stride, i);
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) err |= kErrVertex;
  }
  if (i < n_tri) {
    const int a = tri[3 * (size_t)i], b = tri[3 * (size_t)i + 1], c = tri[3 * (size_t)i + 2];
    double A = 0.0;
    if (a < 0 || a >= n_vert || b < 0 || b >= n_vert || c < 0 || c >= n_vert) {
      err |= kErrIndex;
    } else {
      const V3 p0 = vertex_at(vert, stride, a), p1 = vertex_at(vert, stride, b), p2 = vertex_at(vert, stride, c);
      const double e1x = __dsub_rn((double)p1.x, (double)p0.x), e1y = __dsub_rn((double)p1.y, (double)p0.y),
                   e1z = __dsub_rn((double)p1.z, (double)p0.z);
      const double e2x = __dsub_rn((double)p2.x, (double)p0.x), e2y = __dsub_rn((double)p2.y, (double)p0.y),
                   e2z = __dsub_rn((double)p2.z, (double)p0.z);
      const double x = __dsub_rn(__dmul_rn(e1y, e2z), __dmul_rn(e1z, e2y));
      const double y = __dsub_rn(__dmul_rn(e1z, e2x), __dmul_rn(e1x, e2z));
      const double z = __dsub_rn(__dmul_rn(e1x, e2y), __dmul_rn(e1y, e2x));
      A = __dmul_rn(0.5, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z))));
      if (!(A >= 0.0 && A <= DBL_MAX)) A = 0.0;   // a non-finite vertex: flagged above or by its own thread
    }
    area[i] = A;
    if (A > 0.0) atomicMax(&meta->amax_bits, (unsigned long long)__double_as_longlong(A));
  }
  if (err) atomicOr(&meta->err, err);
}

__global__ __launch_bounds__(256) void prep_weights(const double* __restrict__ area, int n_tri,
                                                    const SampleMeta* __restrict__ meta, unsigned long long* __restrict__ w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tri) return;
  const double amax = __longlong_as_double((long long)meta->amax_bits);
  w[i] = amax > 0.0 ? (unsigned long long)floor(__dmul_rn(__ddiv_rn(area[i], amax), 4294967296.0)) : 0ull;
}

// one sample per thread; xyz4 (nullable): the positions again as float4 {x, y, z, 0}, what the farthest-point kernels read
__global__ __launch_bounds__(256) void prep_sample(const float* __restrict__ vert, int stride, const int* __restrict__ tri,
                                                   int n_tri, const unsigned long long* __restrict__ C,
                                                   const SampleMeta* __restrict__ meta, unsigned long long seed, int n_samples,
                                                   float* __restrict__ xyz, float* __restrict__ nrm, int* __restrict__ tri_out,
                                                   float4* __restrict__ xyz4) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_samples) return;
  const unsigned long long W = C[n_tri - 1];
  if (W == 0ull || meta->err) return;   // (the host reports it)
  const unsigned long long state = sample_state(seed, s);
  const unsigned long long r = ((unsigned long long)sample_variate(state, 0) << 31) | (unsigned long long)sample_variate(state, 1);
  // (r W) >> 62: r < 2^62 and W < 2^55, so the high word stays below 2^53
  const unsigned long long target = (__umul64hi(r, W) << 2) | ((r * W) >> 62);
  int lo = 0, hi = n_tri - 1;   // the first t with C[t] > target; C[n_tri - 1] = W > target
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (C[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  const int t = lo;
  const V3 p0 = vertex_at(vert, stride, tri[3 * (size_t)t]), p1 = vertex_at(vert, stride, tri[3 * (size_t)t + 1]),
           p2 = vertex_at(vert, stride, tri[3 * (size_t)t + 2]);
  const float two_m31 = 4.656612873077392578125e-10f;
  float a = exact::mul(__uint2float_rn(sample_variate(state, 2)), two_m31);
  float b = exact::mul(__uint2float_rn(sample_variate(state, 3)), two_m31);
  if (exact::add(a, b) > 1.f) {
    a = exact::sub(1.f, a);
    b = exact::sub(1.f, b);
  }
  const V3 e1 = exact::vsub(p1, p0), e2 = exact::vsub(p2, p0);
  const V3 p = {exact::add(exact::add(p0.x, exact::mul(a, e1.x)), exact::mul(b, e2.x)),
                exact::add(exact::add(p0.y, exact::mul(a, e1.y)), exact::mul(b, e2.y)),
                exact::add(exact::add(p0.z, exact::mul(a, e1.z)), exact::mul(b, e2.z))};
  xyz[3 * (size_t)s] = p.x;
  xyz[3 * (size_t)s + 1] = p.y;
  xyz[3 * (size_t)s + 2] = p.z;
  if (xyz4) xyz4[s] = make_float4(p.x, p.y, p.z, 0.f);
  if (nrm) {
    const V3 nn = exact::normalized(exact::cross(e1, e2));
    nrm[3 * (size_t)s] = nn.x;
    nrm[3 * (size_t)s + 1] = nn.y;
    nrm[3 * (size_t)s + 2] = nn.z;
  }
  if (tri_out) tri_out[s] = t;
}

// ---------------------------------------------------------------------------------------------------- farthest points

constexpr int kResThreads = 1024, kResWaves = kResThreads / 64, kResSlots = 16;
constexpr int kMultiThreads = 256, kMultiWaves = kMultiThreads / 64, kMultiGroups = 256;

__device__ __forceinline__ unsigned long long d_key(float d, int index) {   // d >= 0
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(~(unsigned int)index);
}
// the key of "largest x, ties the lowest index": x's bit pattern made to order as the floats do (-0 counts as +0)
__device__ __forceinline__ unsigned long long x_key(float x, int index) {
  const unsigned int u = __float_as_uint(x + 0.f);
  const unsigned int o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)o << 32) | (unsigned long long)(~(unsigned int)index);
}
// (key 0: nothing left to pick -- only a cloud of non-finite points gets there -- reads as index 0, never out of bounds)
__device__ __forceinline__ int key_index(unsigned long long key) { return key ? (int)(~(unsigned int)key) : 0; }

struct WaveRec {   // what a wave leaves per pick: its best key and that point
  unsigned long long key;
  float x, y, z, pad;
  float pad2[2];
};

// The resident form; S = points per thread (1, 2, 4, 8, 16).  One workgroup.
template <int S>
__global__ __launch_bounds__(kResThreads) void fps_resident(const float4* __restrict__ P, int n, int k, int start,
                                                            int* __restrict__ order, float* __restrict__ radius2) {
  __shared__ WaveRec s_rec[2][kResWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float px[S], py[S], pz[S], d[S];
#pragma unroll
  for (int j = 0; j < S; ++j) {
    // (no branch around the writes: the arrays stay sixteen registers each, not one vector copied per branch)
    const int i = t + kResThreads * j;
    const bool in = i < n;
    const float4 v = P[in ? i : 0];
    px[j] = in ? v.x : 0.f;
    py[j] = in ? v.y : 0.f;
    pz[j] = in ? v.z : 0.f;
    d[j] = in ? INFINITY : -1.f;   // (outside the cloud: never picked, like a picked point)
  }
  int bank = 0;
  // the pick of one round: every lane's candidate {key, point} -> the workgroup's best, in every lane
  const auto block_best = [&](unsigned long long key, float bx, float by, float bz, float& cx, float& cy, float& cz) {
    const unsigned long long wk = wave::max(key);
    if (key == wk && (key != 0ull || lane == 0)) s_rec[bank][wave] = WaveRec{wk, bx, by, bz, 0.f, {0.f, 0.f}};
    __syncthreads();
    unsigned long long best = 0ull;
    int w = 0;
#pragma unroll
    for (int q = 0; q < kResWaves; ++q) {
      const unsigned long long o = s_rec[bank][q].key;
      if (o > best) {
        best = o;
        w = q;
      }
    }
    cx = s_rec[bank][w].x;
    cy = s_rec[bank][w].y;
    cz = s_rec[bank][w].z;
    bank ^= 1;
    return best;
  };

  float cx, cy, cz;
  int pick;
  {   // pick 0: `start`, or the largest x
    unsigned long long key = 0ull;
    float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int i = t + kResThreads * j;
      if (i >= n) continue;
      const unsigned long long kj = start < 0 ? x_key(px[j], i) : (i == start ? ~0ull : 0ull);
      if (kj > key) {
        key = kj;
        bx = px[j];
        by = py[j];
        bz = pz[j];
      }
    }
    if (start >= 0 && key != 0ull) key = d_key(FLT_MAX, start);
    const unsigned long long best = block_best(key, bx, by, bz, cx, cy, cz);
    pick = key_index(best);
    if (t == 0) {
      order[0] = pick;
      if (radius2) radius2[0] = FLT_MAX;
    }
  }
  for (int r = 1; r < k; ++r) {
    float bd = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int i = t + kResThreads * j;
      const float nd = exact::sqnorm_lr(V3{exact::sub(px[j], cx), exact::sub(py[j], cy), exact::sub(pz[j], cz)});
      float dj = nd < d[j] ? nd : d[j];
      if (i == pick) dj = -1.f;
      d[j] = dj;
      if (dj > bd) {   // strict: the lowest index of a lane's ties (i ascends with j)
        bd = dj;
        bi = i;
        bx = px[j];
        by = py[j];
        bz = pz[j];
      }
    }
    const unsigned long long key = bd >= 0.f ? d_key(bd, bi) : 0ull;
    const unsigned long long best = block_best(key, bx, by, bz, cx, cy, cz);
    pick = key_index(best);
    if (t == 0) {
      order[r] = pick;
      if (radius2) radius2[r] = __uint_as_float((unsigned int)(best >> 32));
    }
  }
}

// the workgroup's max of one key per thread, in every thread (kMultiThreads threads; s: kMultiWaves words of LDS)
__device__ __forceinline__ unsigned long long multi_block_max(unsigned long long key, unsigned long long* s) {
  const unsigned long long wk = wave::max(key);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = wk;
  __syncthreads();
  unsigned long long best = s[0];
#pragma unroll
  for (int q = 1; q < kMultiWaves; ++q) best = s[q] > best ? s[q] : best;
  return best;
}

// Launch 0 of the multi-launch form: d = inf, and the partial keys that make pick 0 (`start`, or the largest x).
__global__ __launch_bounds__(kMultiThreads) void fps_multi_init(const float4* __restrict__ P, int n, int L, int start,
                                                                float* __restrict__ d, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_a[kMultiWaves];
  const int g = blockIdx.x, lo = g * L, hi = min(n, lo + L);
  unsigned long long key = 0ull;
  for (int i = lo + (int)threadIdx.x; i < hi; i += kMultiThreads) {
    d[i] = INFINITY;
    const unsigned long long ki = start < 0 ? x_key(P[i].x, i) : (i == start ? d_key(FLT_MAX, i) : 0ull);
    key = ki > key ? ki : key;
  }
  const unsigned long long best = multi_block_max(key, s_a);
  if (threadIdx.x == 0) part[g] = best;
}

// Launch r + 1: pick r out of part_in, then (unless it was the last pick) the slice's update and its key into part_out.
__global__ __launch_bounds__(kMultiThreads) void fps_multi_pick(const float4* __restrict__ P, int n, int L, int G, int r, int last,
                                                                float* __restrict__ d, const unsigned long long* __restrict__ part_in,
                                                                unsigned long long* __restrict__ part_out, int* __restrict__ order,
                                                                float* __restrict__ radius2) {
  __shared__ unsigned long long s_a[kMultiWaves], s_b[kMultiWaves];
  const int g = blockIdx.x, lo = g * L, hi = min(n, lo + L);
  const unsigned long long won = multi_block_max((int)threadIdx.x < G ? part_in[threadIdx.x] : 0ull, s_a);
  const int pick = key_index(won);
  if (g == 0 && threadIdx.x == 0) {
    order[r] = pick;
    if (radius2) radius2[r] = r == 0 ? FLT_MAX : __uint_as_float((unsigned int)(won >> 32));
  }
  if (last) return;
  const float4 c = P[pick];
  unsigned long long key = 0ull;
  for (int i = lo + (int)threadIdx.x; i < hi; i += kMultiThreads) {
    const float4 p = P[i];
    const float nd = exact::sqnorm_lr(V3{exact::sub(p.x, c.x), exact::sub(p.y, c.y), exact::sub(p.z, c.z)});
    const float di = d[i];
    float dn = nd < di ? nd : di;
    if (i == pick) dn = -1.f;
    d[i] = dn;
    const unsigned long long ki = dn >= 0.f ? d_key(dn, i) : 0ull;
    key = ki > key ? ki : key;
  }
  const unsigned long long best = multi_block_max(key, s_b);
  if (threadIdx.x == 0) part_out[g] = best;
}

// rows order[0 .. m) of the dense sample into the caller's arrays
__global__ __launch_bounds__(256) void prep_gather(const int* __restrict__ order, int m, const float* __restrict__ xyz,
                                                   const float* __restrict__ nrm, const int* __restrict__ tri,
                                                   float* __restrict__ xyz_out, float* __restrict__ nrm_out, int* __restrict__ tri_out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const size_t i = (size_t)order[r];
  for (int q = 0; q < 3; ++q) {
    xyz_out[3 * (size_t)r + q] = xyz[3 * i + q];
    nrm_out[3 * (size_t)r + q] = nrm[3 * i + q];
  }
  tri_out[r] = tri[i];
}

__global__ __launch_bounds__(256) void prep_pad4(const float* __restrict__ xyz, int n, float4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.f);
}

bool fps_force_multi() {   // read at every call: the tests change it between calls
  const char* v = getenv("PGP_FPS_FORM");
  return v && !strcmp(v, "multi");
}

}  // namespace

int launch_sample_mesh(pgp_ctx* ctx, const float* d_vert, int n_vert, int stride, const int* d_tri, int n_tri, int n_samples,
                       unsigned long long seed, float* d_xyz, float* d_nrm, int* d_tri_out, float4* d_xyz4, hipStream_t st) {
  size_t scan_bytes = 0;
  hipError_t he = rocprim::inclusive_scan(nullptr, scan_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                          (size_t)n_tri, rocprim::plus<unsigned long long>(), st);
  if (he != hipSuccess) {
    set_error("rocprim::inclusive_scan (size query) failed: %s", hipGetErrorString(he));
    return PGP_EHIP;
  }
  Carve cv;
  const auto c_meta = cv.add<SampleMeta>(1, 256);
  const auto c_area = cv.add<double>((size_t)n_tri, 256);
  const auto c_w = cv.add<unsigned long long>((size_t)n_tri, 256);
  const auto c_C = cv.add<unsigned long long>((size_t)n_tri, 256);
  const auto c_scan = cv.add<unsigned char>(scan_bytes + 16, 256);
  int rc = cv.ensure(ctx->d_prep_ws);
  if (rc != PGP_OK) return rc;
  SampleMeta* meta = cv.at(c_meta);
  PGP_HIP(hipMemsetAsync(meta, 0, sizeof(SampleMeta), st));
  const int n_both = std::max(n_tri, n_vert);
  hipLaunchKernelGGL(prep_areas, dim3((n_both + 255) / 256), dim3(256), 0, st, d_vert, n_vert, stride, d_tri, n_tri, cv.at(c_area),
                     meta);
  hipLaunchKernelGGL(prep_weights, dim3((n_tri + 255) / 256), dim3(256), 0, st, (const double*)cv.at(c_area), n_tri,
                     (const SampleMeta*)meta, cv.at(c_w));
  he = rocprim::inclusive_scan(cv.at(c_scan), scan_bytes, cv.at(c_w), cv.at(c_C), (size_t)n_tri,
                               rocprim::plus<unsigned long long>(), st);
  if (he != hipSuccess) {
    set_error("rocprim::inclusive_scan failed: %s", hipGetErrorString(he));
    return PGP_EHIP;
  }
  hipLaunchKernelGGL(prep_sample, dim3((n_samples + 255) / 256), dim3(256), 0, st, d_vert, stride, d_tri, n_tri,
                     (const unsigned long long*)cv.at(c_C), (const SampleMeta*)meta, seed, n_samples, d_xyz, d_nrm, d_tri_out, d_xyz4);
  PGP_HIP(hipGetLastError());
  // the one synchronisation: the error flag and the largest area
  SampleMeta hm{};
  PGP_HIP(hipMemcpyAsync(&hm, meta, sizeof hm, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  if (hm.err & kErrIndex) {
    set_error("pgp_sample_mesh: a triangle names a vertex outside [0, %d)", n_vert);
    return PGP_EINVAL;
  }
  if (hm.err & kErrVertex) {
    set_error("pgp_sample_mesh: a vertex is NaN or infinite");
    return PGP_EINVAL;
  }
  if (hm.amax_bits == 0ull) {
    set_error("pgp_sample_mesh: every triangle has zero area");
    return PGP_EINVAL;
  }
  return PGP_OK;
}

int launch_farthest_points(pgp_ctx* ctx, const float4* d_xyz4, int n, int k, int start, int* d_order, float* d_radius2,
                           hipStream_t st) {
  if (n <= kResThreads * kResSlots && !fps_force_multi()) {
    const int per = (n + kResThreads - 1) / kResThreads;
    const dim3 grid(1), block(kResThreads);
    if (per <= 1) hipLaunchKernelGGL(fps_resident<1>, grid, block, 0, st, d_xyz4, n, k, start, d_order, d_radius2);
    else if (per <= 2) hipLaunchKernelGGL(fps_resident<2>, grid, block, 0, st, d_xyz4, n, k, start, d_order, d_radius2);
    else if (per <= 4) hipLaunchKernelGGL(fps_resident<4>, grid, block, 0, st, d_xyz4, n, k, start, d_order, d_radius2);
    else if (per <= 8) hipLaunchKernelGGL(fps_resident<8>, grid, block, 0, st, d_xyz4, n, k, start, d_order, d_radius2);
    else hipLaunchKernelGGL(fps_resident<kResSlots>, grid, block, 0, st, d_xyz4, n, k, start, d_order, d_radius2);
    PGP_HIP(hipGetLastError());
    return PGP_OK;
  }
  // slices of L points over G workgroups (the last slice may be short, never empty)
  const int G0 = std::min(kMultiGroups, (n + kMultiThreads - 1) / kMultiThreads);
  const int L = (n + G0 - 1) / G0;
  const int G = (n + L - 1) / L;
  Carve cv;
  const auto c_d = cv.add<float>((size_t)n, 256);
  const auto c_part = cv.add<unsigned long long>(2 * (size_t)kMultiGroups, 256);
  const int rc = cv.ensure(ctx->d_fps_ws);
  if (rc != PGP_OK) return rc;
  float* d = cv.at(c_d);
  unsigned long long* part = cv.at(c_part);
  hipLaunchKernelGGL(fps_multi_init, dim3(G), dim3(kMultiThreads), 0, st, d_xyz4, n, L, start, d, part);
  for (int r = 0; r < k; ++r)
    hipLaunchKernelGGL(fps_multi_pick, dim3(G), dim3(kMultiThreads), 0, st, d_xyz4, n, L, G, r, r == k - 1 ? 1 : 0, d,
                       (const unsigned long long*)(part + (size_t)(r & 1) * kMultiGroups),
                       part + (size_t)((r + 1) & 1) * kMultiGroups, d_order, d_radius2);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

int launch_pad4(const float* d_xyz, int n, float4* d_out, hipStream_t st) {
  hipLaunchKernelGGL(prep_pad4, dim3((n + 255) / 256), dim3(256), 0, st, d_xyz, n, d_out);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

int launch_model_gather(const int* d_order, int m, const float* d_xyz, const float* d_nrm, const int* d_tri, float* d_xyz_out,
                        float* d_nrm_out, int* d_tri_out, hipStream_t st) {
  hipLaunchKernelGGL(prep_gather, dim3((m + 255) / 256), dim3(256), 0, st, d_order, m, d_xyz, d_nrm, d_tri, d_xyz_out, d_nrm_out,
                     d_tri_out);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

}  // namespace pgp
