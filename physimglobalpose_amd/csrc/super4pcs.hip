// csrc/super4pcs.hip -- the matcher's classic mode (operMode 0, "Super4PCS") on gfx950: positions alone, wide planar bases,
// two pair lists per base.
//
// Replaces
//   Match4PCSBase::SelectQuadrilateral         S4/algorithms/match4pcsBase.cc:505-580
//     + SelectRandomTriangle                   :377-410      (base_device.h: the rule v4pcs.hip uses)
//     + TryQuadrilateral                       :415-464      (base_device.h: the function base_select.hip uses)
//   the two ExtractPairs calls per base        :1963-1969    for MANY distances at once, the lists left on the device
//
// Base: a workgroup per attempt.  The triangle trials are strided over its 256 threads; the arg-max key (width bits << 32 |
// ~trial) is reduced over the waves and then over LDS.  The plane through the triangle (double arithmetic, narrowed to
// float as the reference's Scalar) gives every scene point its planar distance |A x + B y + C z - 1|; the fourth point is
// the workgroup arg-min of (distance bits << 32 | index) over the points that keep the `too_small` clearance from all three:
// the smallest distance, then the lowest index -- the reference's strict `<` walking upward.  TryQuadrilateral then runs on
// twelve lanes of wave 0.
//
// Pair lists: list k holds what pair_rows (congruent.hip) returns for dist[k] -- (j, i) then (i, j) for every i > j with
// !(| |q_i - q_j| - d | > eps), in (i, j) order.  A wave per (row i, chunk of 64 lists): every |q_i - q_j| of a 64-column
// tile is computed once and tested against each distance of the chunk by ballot; lane k of the wave keeps list k's running
// count (count pass) or output position (fill pass).  Count, prefix sums over the rows of a list, fill: the same kernel
// twice.  Plain launches, no workgroup waits for another, every loop bounded by its input.  Every result is an integer or
// a float made of separately rounded operations.

#include "pgp_internal.h"
#include "base_device.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace pgp {

namespace {

using namespace exact;   // exact_f32.h

// ---------------- SelectQuadrilateral: a workgroup per attempt ----------------
constexpr int kBaseThreads = 256;

__global__ __launch_bounds__(kBaseThreads) void wide_bases(const float4* __restrict__ P, int n, unsigned long long seed, int T,
                                                           float D, float too_small, int4* __restrict__ ids,
                                                           float2* __restrict__ inv, float2* __restrict__ dist,
                                                           int* __restrict__ status, float* __restrict__ xyz) {
  __shared__ unsigned long long s_max[kBaseThreads / 64], s_min[kBaseThreads / 64];
  const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long st = sample_state(seed, a);
  const unsigned un = (unsigned)n;
  const int i0 = (int)(sample_variate(st, 0) % un);
  const V3 p0 = ld3(P, i0);
  const float DD = mul(D, D);
  // the widest triangle (base_device.h): trials strided over the workgroup
  unsigned long long best = v4dev::wave_max(v4dev::widest_triangle(P, un, st, T, DD, p0, tid, kBaseThreads));
  if (lane == 0) s_max[wave] = best;
  __syncthreads();
  best = s_max[0];
#pragma unroll
  for (int w = 1; w < kBaseThreads / 64; ++w) best = s_max[w] > best ? s_max[w] : best;
  // the fourth point: the most planar scene point that is not too close to the three (base.cc:527-565)
  int i1 = -1, i2 = -1;
  unsigned long long mine = ~0ull;
  if (best != 0ull) {
    const int i = v4dev::triangle_trial(best);
    i1 = (int)(sample_variate(st, 1 + 2 * i) % un);
    i2 = (int)(sample_variate(st, 2 + 2 * i) % un);
    const V3 p1 = ld3(P, i1), p2 = ld3(P, i2);
    const ppfk::Plane pl = ppfk::fit_plane(p0, p1, p2);
    if (pl.denom != 0.f) {
      for (int k = tid; k < n; k += kBaseThreads) {
        const V3 p = ld3(P, k);
        const V3 e0 = vsub(p, p0), e1 = vsub(p, p1), e2 = vsub(p, p2);
        if (sqnorm_lr(e0) >= too_small && sqnorm_lr(e1) >= too_small && sqnorm_lr(e2) >= too_small) {
          // Scalar distance = std::abs(A x + B y + C z - 1.0): float products and sums, double minus
          const float lin = add(add(mul(pl.A, p.x), mul(pl.B, p.y)), mul(pl.C, p.z));
          const float planar = (float)fabs((double)lin - 1.0);
          if (planar < FLT_MAX) {   // strict `<` from FLT_MAX: NaN and +inf never win (planar >= 0: its bits order as floats)
            const unsigned long long key = ((unsigned long long)__float_as_uint(planar) << 32) | (unsigned)k;
            mine = key < mine ? key : mine;
          }
        }
      }
    }
  }
  mine = v4dev::wave_min(mine);
  if (lane == 0) s_min[wave] = mine;
  __syncthreads();
  if (wave != 0) return;
  mine = s_min[0];
#pragma unroll
  for (int w = 1; w < kBaseThreads / 64; ++w) mine = s_min[w] < mine ? s_min[w] : mine;
  int4 out = make_int4(-1, -1, -1, -1);
  float2 o_inv = make_float2(0.f, 0.f), o_dist = make_float2(0.f, 0.f);
  int ok = 0;
  if (mine != ~0ull) {   // (uniform over the wave)
    int q[4] = {i0, i1, i2, (int)(unsigned)(mine & 0xFFFFFFFFull)};
    float f1 = 0.f, f2 = 0.f;
    if (ppfk::try_quadrilateral(P, q, &f1, &f2)) {
      out = make_int4(q[0], q[1], q[2], q[3]);
      o_inv = make_float2(f1, f2);
      // distance1 / distance6 of base.cc:1952-1953: Eigen's norm, x x + (y y + z z)
      o_dist = make_float2(norm_eigen(vsub(ld3(P, q[0]), ld3(P, q[1]))),
                           norm_eigen(vsub(ld3(P, q[2]), ld3(P, q[3]))));
      ok = 1;
    }
  }
  if (lane == 0) {
    ids[a] = out;
    inv[a] = o_inv;
    dist[a] = o_dist;
    status[a] = ok;
  }
  // the base's positions in its final order (the join's cones are made from them on the host); zeros where there is none
  if (lane < 4) {
    const int id = lane == 0 ? out.x : (lane == 1 ? out.y : (lane == 2 ? out.z : out.w));
    const float4 p = ok ? P[id] : make_float4(0.f, 0.f, 0.f, 0.f);
    float* o = xyz + 12 * (size_t)a + 3 * lane;
    o[0] = p.x;
    o[1] = p.y;
    o[2] = p.z;
  }
}

// ---------------- ExtractPairs for many distances ----------------
constexpr int kListChunk = 64;   // lists per wave: lane k keeps the counter of list k of the chunk

// FILL = false: row_cnt[list * n + i] = hits of row i in that list.  FILL = true: writes them, (j, i) then (i, j), from pair
// list_off[list] + 2 * row_start[list * n + i] of `out` on.
template <bool FILL>
__global__ __launch_bounds__(256) void pair_lists(const float4* __restrict__ Q, int n, const float* __restrict__ dist, int nl,
                                                  double eps, uint32_t* __restrict__ row_cnt,
                                                  const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ list_off,
                                                  int2* __restrict__ out) {
  const int n_chunks = (nl + kListChunk - 1) / kListChunk;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wv >= (long long)n * n_chunks) return;
  const int i = (int)(wv / n_chunks), k0 = (int)(wv % n_chunks) * kListChunk;
  const int kn = min(kListChunk, nl - k0);
  const bool has = lane < kn;   // this lane keeps list k0 + lane
  const size_t my_row = (size_t)(k0 + lane) * (size_t)n + (size_t)i;
  // count pass: hits so far; fill pass: the next output position of the list, in pairs
  uint32_t mine = (FILL && has) ? list_off[k0 + lane] + 2u * row_start[my_row] : 0u;
  const V3 qi = ld3(Q, i);
  for (int j0 = 0; j0 < i; j0 += 64) {
    const int j = j0 + lane;
    const bool live = j < i;
    // (q.pos() - p.pos()).norm() as pair_rows has it: q_i - q_j, x x + (y y + z z), correctly rounded sqrt
    const double dij = live ? (double)norm_eigen(vsub(qi, ld3(Q, j))) : 0.0;
    for (int k = 0; k < kn; ++k) {
      const double dk = (double)dist[k0 + k];
      const bool hit = live && !(fabs(dij - dk) > eps);
      const unsigned long long m = __ballot(hit);
      if (m == 0ull) continue;
      const uint32_t cnt = (uint32_t)__popcll(m);
      if (FILL) {
        const uint32_t at = __shfl(mine, k, 64) + 2u * (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (hit) {
          out[at] = make_int2(j, i);        // pairs->emplace_back(j, i)
          out[at + 1] = make_int2(i, j);    // pairs->emplace_back(i, j)
        }
      }
      if (lane == k) mine += FILL ? 2u * cnt : cnt;
    }
  }
  if (!FILL && has) row_cnt[my_row] = mine;
}

// exclusive prefix sums over the n rows of every list: one workgroup per list, a run of rows per thread
__global__ __launch_bounds__(256) void list_row_starts(const uint32_t* __restrict__ row_cnt, int n, uint32_t* __restrict__ row_start,
                                                       uint32_t* __restrict__ totals) {
  __shared__ uint32_t s_sum[256];
  const int l = blockIdx.x, tid = threadIdx.x;
  const int per = (n + 255) / 256, lo = min(tid * per, n), hi = min(lo + per, n);
  const uint32_t* cnt = row_cnt + (size_t)l * n;
  uint32_t sum = 0u;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  s_sum[tid] = sum;
  __syncthreads();
  uint32_t run = 0u;
  for (int t = 0; t < tid; ++t) run += s_sum[t];
  for (int i = lo; i < hi; ++i) {
    row_start[(size_t)l * n + i] = run;
    run += cnt[i];
  }
  if (tid == 255) totals[l] = run;   // the last thread's running sum is the list's total
}

constexpr size_t kRowWordsMax = (size_t)1 << 28;   // lists x rows of one batch (two uint32 arrays of that many words)

}  // namespace

int launch_wide_bases(pgp_ctx* ctx, unsigned long long seed, int n_attempts, int triangle_trials, float max_base_diameter,
                      int* h_ids, float* h_inv, float* h_dist, int* h_status, float* h_xyz, hipStream_t st) {
  if (ctx->nP <= 0 || !ctx->d_P.p) {
    set_error("no scene: call pgp_set_scene first");
    return PGP_ESTATE;
  }
  const size_t A = (size_t)n_attempts;
  Carve c;
  const auto p_ids = c.add<int4>(A, 16);
  const auto p_inv = c.add<float2>(A, 16);
  const auto p_dist = c.add<float2>(A, 16);
  const auto p_status = c.add<int>(A, 16);
  const auto p_xyz = c.add<float>(12 * A, 16);
  int rc = c.ensure(ctx->d_s4_sel);
  if (rc != PGP_OK) return rc;
  // const Scalar too_small = std::pow(max_base_diameter_ * kBaseTooSmall, 2): a float product, squared in double, narrowed
  const float scaled = max_base_diameter * 0.1f;
  const float too_small = (float)std::pow((double)scaled, 2);
  hipLaunchKernelGGL(wide_bases, dim3((unsigned)n_attempts), dim3(kBaseThreads), 0, st, (const float4*)ctx->d_P.as<float4>(), ctx->nP,
                     seed, triangle_trials, max_base_diameter, too_small, c.at(p_ids), c.at(p_inv), c.at(p_dist), c.at(p_status),
                     c.at(p_xyz));
  PGP_HIP(hipGetLastError());
  HostOut out(ctx, st);
  if ((rc = out.to(h_ids, c.at(p_ids), p_ids.bytes())) != PGP_OK || (rc = out.to(h_inv, c.at(p_inv), p_inv.bytes())) != PGP_OK ||
      (rc = out.to(h_dist, c.at(p_dist), p_dist.bytes())) != PGP_OK || (rc = out.to(h_status, c.at(p_status), p_status.bytes())) != PGP_OK ||
      (h_xyz && (rc = out.to(h_xyz, c.at(p_xyz), p_xyz.bytes())) != PGP_OK))
    return rc;
  return out.sync();
}

// The pair lists of nl distances, left in ctx->d_s4_pairs with their offsets in ctx->s4_off (pairs).  h_n_pairs[nl]: pairs per list.
int launch_extract_pairs_batch(pgp_ctx* ctx, const float* h_dist, int nl, float eps, int* h_n_pairs, hipStream_t st) {
  const int n = ctx->nQs;
  if (n <= 0 || !ctx->d_Qs.p) {
    set_error("no search model: call pgp_set_search_model first");
    return PGP_ESTATE;
  }
  // the lists are rewritten below: a quad batch built from them names pairs that are about to go
  ctx->s4_nl = 0;
  ctx->s4_off.clear();
  if (ctx->csb_lists) {
    ctx->csb_nb = 0;
    ctx->csb_fit_m = 0;
  }
  if (n > 65536 || (size_t)nl * (size_t)n > kRowWordsMax) {
    set_error("pgp_extract_pairs_batch: %d lists over %d points exceed the batch's row counters (%zu words, 65536 points)", nl, n,
              kRowWordsMax);
    return PGP_EINVAL;
  }
  if (nl == 0) {
    ctx->s4_off.assign(1, 0u);
    return PGP_OK;
  }
  const size_t L = (size_t)nl, rows = L * (size_t)n;
  Carve c;
  const auto p_dist = c.add<float>(L, 16);
  const auto p_tot = c.add<uint32_t>(L, 16);
  const auto p_off = c.add<uint32_t>(L, 16);
  const auto p_cnt = c.add<uint32_t>(rows, 16);
  const auto p_start = c.add<uint32_t>(rows, 16);
  int rc = c.ensure(ctx->d_s4_ws);
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(c.at(p_dist), h_dist, p_dist.bytes(), hipMemcpyHostToDevice, st));
  const float4* Q = ctx->d_Qs.as<float4>();
  const long long waves = (long long)n * ((nl + kListChunk - 1) / kListChunk);
  const dim3 grid((unsigned)((waves + 3) / 4));
  hipLaunchKernelGGL(pair_lists<false>, grid, dim3(256), 0, st, Q, n, (const float*)c.at(p_dist), nl, (double)eps, c.at(p_cnt),
                     (const uint32_t*)nullptr, (const uint32_t*)nullptr, (int2*)nullptr);
  hipLaunchKernelGGL(list_row_starts, dim3((unsigned)nl), dim3(256), 0, st, (const uint32_t*)c.at(p_cnt), n, c.at(p_start), c.at(p_tot));
  PGP_HIP(hipGetLastError());
  std::vector<uint32_t> hits(L);
  PGP_HIP(hipMemcpyAsync(hits.data(), c.at(p_tot), p_tot.bytes(), hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  std::vector<uint32_t> off(L + 1, 0u);
  unsigned long long total = 0ull;
  for (size_t k = 0; k < L; ++k) {
    const unsigned long long pairs = 2ull * hits[k];
    if (pairs >= (1ull << 24)) {   // the join's keys hold a pair index in 24 bits
      set_error("pgp_extract_pairs_batch: list %zu holds %llu pairs (fewer than 2^24 fit the join's keys)", k, pairs);
      return PGP_EINVAL;
    }
    off[k] = (uint32_t)total;
    total += pairs;
    if (total >= (1ull << 31)) {
      set_error("pgp_extract_pairs_batch: more than 2^31 pairs in one batch");
      return PGP_EINVAL;
    }
  }
  off[L] = (uint32_t)total;
  if ((rc = ctx->d_s4_pairs.ensure(std::max<size_t>((size_t)total, 1) * 8)) != PGP_OK) return rc;
  if (total > 0) {
    PGP_HIP(hipMemcpyAsync(c.at(p_off), off.data(), p_off.bytes(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pair_lists<true>, grid, dim3(256), 0, st, Q, n, (const float*)c.at(p_dist), nl, (double)eps, (uint32_t*)nullptr,
                       (const uint32_t*)c.at(p_start), (const uint32_t*)c.at(p_off), ctx->d_s4_pairs.as<int2>());
    PGP_HIP(hipGetLastError());
    PGP_HIP(hipStreamSynchronize(st));   // (`off` is the source of a copy queued above)
  }
  if (h_n_pairs)
    for (size_t k = 0; k < L; ++k) h_n_pairs[k] = (int)(off[k + 1] - off[k]);
  ctx->s4_off = std::move(off);
  ctx->s4_nl = nl;
  return PGP_OK;
}

int extract_pairs_batch_fetch(pgp_ctx* ctx, int list, int* h_pairs, int cap, int* h_n_pairs, hipStream_t st) {
  if (ctx->s4_nl <= 0 || (int)ctx->s4_off.size() != ctx->s4_nl + 1) {
    set_error("no pair lists: call pgp_extract_pairs_batch first (pgp_set_search_model discards them)");
    return PGP_ESTATE;
  }
  if (list < 0 || list >= ctx->s4_nl) {
    set_error("pgp_extract_pairs_batch_fetch: list %d of %d", list, ctx->s4_nl);
    return PGP_EINVAL;
  }
  const uint32_t lo = ctx->s4_off[list], cnt = ctx->s4_off[list + 1] - lo;
  *h_n_pairs = (int)cnt;
  const size_t n_copy = std::min<size_t>(cnt, (size_t)cap);
  if (n_copy > 0) {
    PGP_HIP(hipMemcpyAsync(h_pairs, ctx->d_s4_pairs.as<int2>() + lo, n_copy * 8, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipStreamSynchronize(st));
  }
  return PGP_OK;
}

}  // namespace pgp
