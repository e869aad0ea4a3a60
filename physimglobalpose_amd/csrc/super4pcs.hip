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
//
// Pair gates (pairCreationFunctor.h:167-253; the fork ships them off and pair_lists has none): pair_lists_gated is the same
// pass with Match4PCSOptions' normal, colour, translation and angle tests between the distance ballot and the output, against
// a record of the list's base edge that base_records gathers from the scene.  The rules are in include/pgp.h.

#include "pgp_internal.h"
#include "wave.h"
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
  unsigned long long best = wave::max(v4dev::widest_triangle(P, un, st, T, DD, p0, tid, kBaseThreads));
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
  mine = wave::min(mine);
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
        const uint32_t at = __shfl(mine, k, 64) + 2u * (uint32_t)wave::rank_in(m, lane);
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

// ---------------- ExtractPairs with the matcher's pair gates (pairCreationFunctor.h:167-253) ----------------
// What a list knows of its base edge (b1, b2): made once per list by base_records, read wave-uniformly in the k loop.
struct BaseRec {
  float4 seg_pna;   // segment1 = (pos_b2 - pos_b1).normalized() | pair_normals_angle = |n_b1 - n_b2|
  float4 p1, p2;    // the two positions
  float4 c1, c2;    // the two colours ((-1, -1, -1): none)
};

// the gates as the kernel reads them: thresholds made on the host, a gate that is off has on_* = 0
struct GateArgs {
  float norm_thr;     // (float)(0.5 * max_normal_difference * M_PI / 180.0)
  float cos_max;      // (float)cos(max_angle * M_PI / 180.0)
  double color_max, trans_max;
  int on_normal, on_color, on_trans, on_angle, directed;
};

__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return {add(a.x, b.x), add(a.y, b.y), add(a.z, b.z)}; }
__device__ __forceinline__ V3 xyz_of(float4 v) { return {v.x, v.y, v.z}; }

__global__ __launch_bounds__(256) void base_records(const float4* __restrict__ P, const float4* __restrict__ Pnw,
                                                    const float4* __restrict__ Prgb /* nullable */, const int2* __restrict__ ids,
                                                    int nl, BaseRec* __restrict__ rec) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nl) return;
  const int2 b = ids[k];   // (checked against the scene's count on the host)
  const V3 p1 = ld3(P, b.x), p2 = ld3(P, b.y);
  const V3 seg = normalized(vsub(p2, p1));
  const float pna = norm_eigen(vsub(ld3(Pnw, b.x), ld3(Pnw, b.y)));
  const float4 none = make_float4(-1.f, -1.f, -1.f, 0.f);
  BaseRec r;
  r.seg_pna = make_float4(seg.x, seg.y, seg.z, pna);
  r.p1 = make_float4(p1.x, p1.y, p1.z, 0.f);
  r.p2 = make_float4(p2.x, p2.y, p2.z, 0.f);
  r.c1 = Prgb ? Prgb[b.x] : none;
  r.c2 = Prgb ? Prgb[b.y] : none;
  rec[k] = r;
}

// a against e1 and b against e2, both strictly nearer than `max` (float norms, compared in double)
__device__ __forceinline__ bool both_within(V3 a, V3 e1, V3 b, V3 e2, double max) {
  return (double)norm_eigen(vsub(a, e1)) < max && (double)norm_eigen(vsub(b, e2)) < max;
}

// pair_lists with the gates.  The same wave per (row i, chunk of 64 lists) and the same distance ballot; what a gate needs of
// the pair alone (|n_q - n_p|, |n_q + n_p|, segment2) is computed once per tile, what it needs of the list is read from the
// list's record where the distance ballot is non-zero.  Two ballots per list, forward (j, i) and backward (i, j): a row's
// counter counts ORDERED pairs.  FILL = false: row_cnt[list * n + i].  FILL = true: writes from pair list_off[list] +
// row_start[list * n + i] of `out` on, (j, i) before (i, j), j ascending.
template <bool FILL>
__global__ __launch_bounds__(256) void pair_lists_gated(const float4* __restrict__ Q, const float4* __restrict__ Qn /* nullable */,
                                                        const float4* __restrict__ Qc /* nullable */, int n,
                                                        const float* __restrict__ dist, const BaseRec* __restrict__ rec, int nl,
                                                        double eps, GateArgs g, uint32_t* __restrict__ row_cnt,
                                                        const uint32_t* __restrict__ row_start,
                                                        const uint32_t* __restrict__ list_off, int2* __restrict__ out) {
  const int n_chunks = (nl + kListChunk - 1) / kListChunk;
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wv >= (long long)n * n_chunks) return;
  const int i = (int)(wv / n_chunks), k0 = (int)(wv % n_chunks) * kListChunk;
  const int kn = min(kListChunk, nl - k0);
  const bool has = lane < kn;   // this lane keeps list k0 + lane
  const size_t my_row = (size_t)(k0 + lane) * (size_t)n + (size_t)i;
  uint32_t mine = (FILL && has) ? list_off[k0 + lane] + row_start[my_row] : 0u;
  const V3 zero = {0.f, 0.f, 0.f}, no_rgb = {-1.f, -1.f, -1.f};
  const V3 qi = ld3(Q, i);
  const V3 ni = Qn ? ld3(Qn, i) : zero;
  const V3 ci = Qc ? ld3(Qc, i) : no_rgb;
  const bool ni_set = sqnorm_eigen(ni) > 0.f;
  for (int j0 = 0; j0 < i; j0 += 64) {
    const int j = j0 + lane;
    const bool live = j < i;
    const int jr = live ? j : 0;   // (a lane past the row reads point 0 and never hits)
    const V3 pj = ld3(Q, jr);      // p = Q[j], q = Q[i]
    const V3 e = vsub(qi, pj);
    const double dij = live ? (double)norm_eigen(e) : 0.0;
    bool n_applies = false;
    double n_first = 0.0, n_second = 0.0;
    if (g.on_normal && Qn) {
      const V3 nj = ld3(Qn, jr);
      n_applies = ni_set && sqnorm_eigen(nj) > 0.f;
      n_first = (double)norm_eigen(vsub(ni, nj));
      n_second = (double)norm_eigen(vadd(ni, nj));
    }
    const V3 cj = (g.on_color && Qc) ? ld3(Qc, jr) : no_rgb;
    const bool pair_rgb = cj.x >= 0.f && ci.x >= 0.f;
    const V3 seg2 = g.on_angle ? normalized(e) : zero;
    const V3 seg2_neg = {-seg2.x, -seg2.y, -seg2.z};
    for (int k = 0; k < kn; ++k) {
      const double dk = (double)dist[k0 + k];
      const bool hit = live && !(fabs(dij - dk) > eps);
      if (__ballot(hit) == 0ull) continue;
      const BaseRec& r = rec[k0 + k];   // wave-uniform
      bool fwd = hit, bwd = hit;
      if (n_applies) {
        const double pna = (double)r.seg_pna.w;
        const double a = fabs(n_first - pna), b = fabs(n_second - pna);
        const float d = (float)(b < a ? b : a);   // std::min(a, b)
        if (d > g.norm_thr) fwd = bwd = false;
      }
      if (g.on_color && pair_rgb && r.c1.x >= 0.f && r.c2.x >= 0.f) {
        const V3 c1 = xyz_of(r.c1), c2 = xyz_of(r.c2);
        const bool good = both_within(cj, c1, ci, c2, g.color_max);
        fwd = fwd && good;
        bwd = bwd && (g.directed ? both_within(ci, c1, cj, c2, g.color_max) : good);
      }
      if (g.on_trans) {
        const V3 b1 = xyz_of(r.p1), b2 = xyz_of(r.p2);
        const bool good = both_within(pj, b1, qi, b2, g.trans_max);
        fwd = fwd && good;
        bwd = bwd && (g.directed ? both_within(qi, b1, pj, b2, g.trans_max) : good);
      }
      if (g.on_angle) {
        const V3 seg1 = xyz_of(r.seg_pna);
        fwd = fwd && dot_eigen(seg1, seg2) >= g.cos_max;
        bwd = bwd && dot_eigen(seg1, seg2_neg) >= g.cos_max;
      }
      const unsigned long long mf = __ballot(fwd), mb = __ballot(bwd);
      if ((mf | mb) == 0ull) continue;
      if (FILL) {
        uint32_t at = __shfl(mine, k, 64) + (uint32_t)wave::rank_in(mf, lane) + (uint32_t)wave::rank_in(mb, lane);
        if (fwd) out[at++] = make_int2(j, i);   // pairs->emplace_back(j, i)
        if (bwd) out[at] = make_int2(i, j);     // pairs->emplace_back(i, j)
      }
      if (lane == k) mine += (uint32_t)__popcll(mf) + (uint32_t)__popcll(mb);
    }
  }
  if (!FILL && has) row_cnt[my_row] = mine;
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
// g == nullptr: pair_lists, every hit is two pairs.  Otherwise pair_lists_gated over the records of h_base_ids[nl][2], whose
// rows count ordered pairs.
static int pair_batch(pgp_ctx* ctx, const char* who, const float* h_dist, const int* h_base_ids, int nl, float eps, const GateArgs* g,
                      int* h_n_pairs, hipStream_t st) {
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
    set_error("%s: %d lists over %d points exceed the batch's row counters (%zu words, 65536 points)", who, nl, n, kRowWordsMax);
    return PGP_EINVAL;
  }
  if (g) {
    if (ctx->nP <= 0 || !ctx->d_P.p) {
      set_error("%s: the gates read the base edges from the scene: call pgp_set_scene first", who);
      return PGP_ESTATE;
    }
    for (int k = 0; k < 2 * nl; ++k)
      if ((unsigned)h_base_ids[k] >= (unsigned)ctx->nP) {
        set_error("%s: base id %d of list %d is outside the scene's %d points", who, h_base_ids[k], k / 2, ctx->nP);
        return PGP_EINVAL;
      }
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
  const auto p_ids = c.add<int2>(g ? L : 0, 16);
  const auto p_rec = c.add<BaseRec>(g ? L : 0, 16);
  int rc = c.ensure(ctx->d_s4_ws);
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(c.at(p_dist), h_dist, p_dist.bytes(), hipMemcpyHostToDevice, st));
  const float4* Q = ctx->d_Qs.as<float4>();
  const float4* Qn = ctx->has_search_normals ? ctx->d_Qs_nrm.as<float4>() : nullptr;
  const float4* Qc = ctx->has_search_colors ? ctx->d_Qs_rgb.as<float4>() : nullptr;
  const long long waves = (long long)n * ((nl + kListChunk - 1) / kListChunk);
  const dim3 grid((unsigned)((waves + 3) / 4));
  if (g) {
    PGP_HIP(hipMemcpyAsync(c.at(p_ids), h_base_ids, p_ids.bytes(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(base_records, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, (const float4*)ctx->d_P.as<float4>(),
                       (const float4*)ctx->d_Pnw.as<float4>(),
                       (const float4*)(ctx->has_scene_colors ? ctx->d_Prgb.as<float4>() : nullptr), (const int2*)c.at(p_ids), nl,
                       c.at(p_rec));
    hipLaunchKernelGGL(pair_lists_gated<false>, grid, dim3(256), 0, st, Q, Qn, Qc, n, (const float*)c.at(p_dist),
                       (const BaseRec*)c.at(p_rec), nl, (double)eps, *g, c.at(p_cnt), (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                       (int2*)nullptr);
  } else {
    hipLaunchKernelGGL(pair_lists<false>, grid, dim3(256), 0, st, Q, n, (const float*)c.at(p_dist), nl, (double)eps, c.at(p_cnt),
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, (int2*)nullptr);
  }
  hipLaunchKernelGGL(list_row_starts, dim3((unsigned)nl), dim3(256), 0, st, (const uint32_t*)c.at(p_cnt), n, c.at(p_start), c.at(p_tot));
  PGP_HIP(hipGetLastError());
  std::vector<uint32_t> hits(L);
  PGP_HIP(hipMemcpyAsync(hits.data(), c.at(p_tot), p_tot.bytes(), hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  std::vector<uint32_t> off(L + 1, 0u);
  unsigned long long total = 0ull;
  for (size_t k = 0; k < L; ++k) {
    const unsigned long long pairs = (g ? 1ull : 2ull) * hits[k];
    if (pairs >= (1ull << 24)) {   // the join's keys hold a pair index in 24 bits
      set_error("%s: list %zu holds %llu pairs (fewer than 2^24 fit the join's keys)", who, k, pairs);
      return PGP_EINVAL;
    }
    off[k] = (uint32_t)total;
    total += pairs;
    if (total >= (1ull << 31)) {
      set_error("%s: more than 2^31 pairs in one batch", who);
      return PGP_EINVAL;
    }
  }
  off[L] = (uint32_t)total;
  if ((rc = ctx->d_s4_pairs.ensure(std::max<size_t>((size_t)total, 1) * 8)) != PGP_OK) return rc;
  if (total > 0) {
    PGP_HIP(hipMemcpyAsync(c.at(p_off), off.data(), p_off.bytes(), hipMemcpyHostToDevice, st));
    if (g)
      hipLaunchKernelGGL(pair_lists_gated<true>, grid, dim3(256), 0, st, Q, Qn, Qc, n, (const float*)c.at(p_dist),
                         (const BaseRec*)c.at(p_rec), nl, (double)eps, *g, (uint32_t*)nullptr, (const uint32_t*)c.at(p_start),
                         (const uint32_t*)c.at(p_off), ctx->d_s4_pairs.as<int2>());
    else
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

int launch_extract_pairs_batch(pgp_ctx* ctx, const float* h_dist, int nl, float eps, int* h_n_pairs, hipStream_t st) {
  return pair_batch(ctx, "pgp_extract_pairs_batch", h_dist, nullptr, nl, eps, nullptr, h_n_pairs, st);
}

int launch_extract_pairs_batch_gated(pgp_ctx* ctx, const float* h_dist, const int* h_base_ids, int nl, float eps,
                                     const pgp_pair_gates* gates, int* h_n_pairs, hipStream_t st) {
  const char* who = "pgp_extract_pairs_batch_gated";
  GateArgs g{};
  if (gates) {
    g.on_normal = gates->max_normal_difference > 0.f;
    g.on_color = gates->max_color_distance > 0.f;
    g.on_trans = gates->max_translation_distance > 0.f;
    g.on_angle = gates->max_angle > 0.f;
    g.directed = gates->directed != 0;
    // const Scalar norm_threshold = 0.5 * options_.max_normal_difference * M_PI / 180.0 (pairCreationFunctor.h:185-186)
    g.norm_thr = (float)(0.5 * (double)gates->max_normal_difference * M_PI / 180.0);
    g.cos_max = (float)std::cos((double)gates->max_angle * M_PI / 180.0);
    g.color_max = (double)gates->max_color_distance;
    g.trans_max = (double)gates->max_translation_distance;
  }
  if (!(g.on_normal || g.on_color || g.on_trans || g.on_angle))   // every gate off: the ungated lists, bit for bit
    return pair_batch(ctx, who, h_dist, nullptr, nl, eps, nullptr, h_n_pairs, st);
  if (nl > 0 && !h_base_ids) {
    set_error("%s: gates are on and base_ids is null", who);
    return PGP_EINVAL;
  }
  return pair_batch(ctx, who, h_dist, h_base_ids, nl, eps, &g, h_n_pairs, st);
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
