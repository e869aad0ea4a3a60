// csrc/v4pcs.hip -- the matcher's tetrahedron-base mode (operMode 2, "V4PCS") on gfx950: positions alone.
//
// Replaces
//   Match4PCSBase::SelectTetrahedronBase       S4/algorithms/match4pcsBase.cc:466-503
//     + SelectRandomTriangle                   :377-410
//   FindCongruentQuadrilateralsV4PCS           :978-1044   (fed by six ExtractPairs calls, :1963-1969, :1998-2020)
//
// Base: a random first point; over T random (second, third) draws the triangle with the largest |u x w| whose two edges
// from the first point are shorter than the base diameter (strict `>` from 0: the first maximum in trial order); over F
// random fourth points the one with the largest |(v1 x v2) . v3| / 6 (strict `>` from 0).  The reference draws from
// rand() seeded from the clock; here the draw is the counter-based one of pgp_internal.h (sample_state / sample_variate),
// a function of (seed, attempt) alone.  A wave per attempt, trials strided over the lanes; the arg-max is a wave
// reduction of the key (value bits << 32 | ~trial): greatest value, then lowest trial.
//
// Join: with the six base distances d1 = |b0 b1|, d2 = |b0 b2|, d3 = |b0 b3|, d4 = |b1 b2|, d5 = |b1 b3|, d6 = |b2 b3| and
// the pair predicate of pair_rows (congruent.hip: a != b and !(|dist(a, b) - d| > eps), float distance, comparison in
// double), (v1, v2, v3, v4) is emitted iff (v1,v2)~d1, (v1,v3)~d2, (v1,v4)~d3, (v2,v3)~d4, (v2,v4)~d5, (v3,v4)~d6.  The
// reference walks six ordered pair lists through hash sets and leaves the output order open; here the six predicates of a
// base are six N x N bit matrices M1..M6 (N <= 4096: a row is at most one 64-bit word per lane of a wave):
//   pass A  a wave per (row i, 64-column tile): every distance is computed once, and for every base of the chunk the six
//           ballots are the row words of M1..M6 (bits past N and the diagonal are zero);
//   pass B  a wave per (base, v1): for every set bit v2 of M1[v1]: C3 = M2[v1] & M4[v2], C4 = M3[v1] & M5[v2]; for every
//           set bit v3 of C3: popcount(C4 & M6[v3]).  Run twice by the same code: count, prefix sums over the rows of a
//           base, fill in (v2, v3, word, bit) order -- ascending (v1, v2, v3, v4), no sort.
// Plain launches, no waiting between workgroups.  Every result is an integer.

#include "pgp_internal.h"
#include "wave.h"
#include "base_device.h"

#include <algorithm>
#include <vector>

namespace pgp {

namespace {

using namespace v4dev;   // base_device.h: exact_f32.h's helpers and the triangle rule shared with super4pcs.hip

// ---------------- SelectTetrahedronBase: a wave per attempt ----------------
__global__ __launch_bounds__(64) void tetra_bases(const float4* __restrict__ P, int n, unsigned long long seed, int T, int F,
                                                  float D, int4* __restrict__ ids, float* __restrict__ dist,
                                                  int* __restrict__ status) {
  const int a = blockIdx.x, lane = threadIdx.x;
  const unsigned long long st = sample_state(seed, a);
  const unsigned un = (unsigned)n;
  const int i0 = (int)(sample_variate(st, 0) % un);
  const V3 p0 = ld3(P, i0);
  const float DD = mul(D, D);
  // the widest triangle (base_device.h): trials strided over the lanes
  unsigned long long best = widest_triangle(P, un, st, T, DD, p0, lane, 64);
  best = wave::max(best);
  int4 out = make_int4(-1, -1, -1, -1);
  int ok = 0;
  float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (best != 0ull) {
    const int i = triangle_trial(best);
    const int i1 = (int)(sample_variate(st, 1 + 2 * i) % un), i2 = (int)(sample_variate(st, 2 + 2 * i) % un);
    const V3 p1 = ld3(P, i1), p2 = ld3(P, i2);
    const V3 n12 = cross(vsub(p1, p0), vsub(p2, p0));
    unsigned long long bestv = 0ull;
    for (int k = lane; k < F; k += 64) {
      const int f = (int)(sample_variate(st, 1 + 2 * T + k) % un);
      const float volume = __fdiv_rn(fabsf(dot_lr(n12, vsub(ld3(P, f), p0))), 6.0f);
      if (volume > 0.f) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(volume) << 32) | (0xFFFFFFFFu - (unsigned)k);
        bestv = key > bestv ? key : bestv;
      }
    }
    bestv = wave::max(bestv);
    if (bestv != 0ull) {
      const int k = (int)(0xFFFFFFFFu - (unsigned)(bestv & 0xFFFFFFFFull));
      const int i3 = (int)(sample_variate(st, 1 + 2 * T + k) % un);
      const V3 p3 = ld3(P, i3);
      out = make_int4(i0, i1, i2, i3);
      ok = 1;
      const V3 e[6] = {vsub(p1, p0), vsub(p2, p0), vsub(p3, p0), vsub(p2, p1), vsub(p3, p1), vsub(p3, p2)};
#pragma unroll
      for (int q = 0; q < 6; ++q) d[q] = norm_lr(e[q]);
    }
  }
  if (lane == 0) {
    ids[a] = out;
    status[a] = ok;
#pragma unroll
    for (int q = 0; q < 6; ++q) dist[6 * (size_t)a + q] = d[q];
  }
}

// ---------------- the join ----------------
// Bit matrices of a chunk of bases: M[(b * 6 + k) * N * W + i * W + c], W = ceil(N / 64) words per row.
// pass A: a wave per (row i, column tile c); four waves per workgroup
__global__ __launch_bounds__(256) void pair_bits(const float4* __restrict__ Q, int N, int W, const float* __restrict__ dist,
                                                 int nb, double eps, unsigned long long* __restrict__ M) {
  const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (wv >= (long long)N * W) return;
  const int i = (int)(wv / W), c = (int)(wv % W);
  const int j = c * 64 + lane;
  const bool live = j < N && j != i;
  double dij = 0.0;
  if (live) {
    // (q_hi - q_lo, as pair_rows subtracts; the squares are the same either way round)
    const V3 d = j < i ? vsub(ld3(Q, i), ld3(Q, j)) : vsub(ld3(Q, j), ld3(Q, i));
    dij = (double)norm_eigen(d);   // the pair predicate's norm, as pair_rows has it: x x + (y y + z z)
  }
  const size_t plane = (size_t)N * W, at = (size_t)i * W + c;
  for (int b = 0; b < nb; ++b) {
    unsigned long long mine = 0ull;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double dk = (double)dist[6 * b + k];
      const unsigned long long m = __ballot(live && !(fabs(dij - dk) > eps));
      if (lane == k) mine = m;
    }
    if (lane < 6) M[((size_t)b * 6 + lane) * plane + at] = mine;
  }
}

__device__ __forceinline__ unsigned long long word_of(unsigned long long mine, int w) { return __shfl(mine, w, 64); }

// pass B: a wave per (base, v1).  FILL = false: row_cnt[b * N + v1] = quads that start with v1.  FILL = true: writes them from
// row_start[b * N + v1] on, up to `cap` quads per base.
template <bool FILL>
__global__ __launch_bounds__(64) void join_rows(const unsigned long long* __restrict__ M, int N, int W,
                                                unsigned long long* __restrict__ row_cnt,
                                                const unsigned long long* __restrict__ row_start, int4* __restrict__ quads,
                                                unsigned long long cap) {
  const int b = blockIdx.x / N, v1 = blockIdx.x % N, lane = threadIdx.x;
  const size_t plane = (size_t)N * W;
  const unsigned long long* M1 = M + ((size_t)b * 6) * plane;
  const unsigned long long *M2 = M1 + plane, *M3 = M2 + plane, *M4 = M3 + plane, *M5 = M4 + plane, *M6 = M5 + plane;
  const bool has = lane < W;
  unsigned long long off = FILL ? row_start[(size_t)b * N + v1] : 0ull;
  if (FILL && off >= cap) return;
  int4* out = FILL ? quads + (size_t)b * cap : nullptr;
  const unsigned long long r1 = has ? M1[(size_t)v1 * W + lane] : 0ull;
  const unsigned long long r2 = has ? M2[(size_t)v1 * W + lane] : 0ull;
  const unsigned long long r3 = has ? M3[(size_t)v1 * W + lane] : 0ull;
  unsigned long long count = 0ull;   // per lane; summed over the wave at the end
  for (int w2 = 0; w2 < W; ++w2) {
    for (unsigned long long bits2 = word_of(r1, w2); bits2; bits2 &= bits2 - 1ull) {
      const int v2 = w2 * 64 + __builtin_ctzll(bits2);
      const unsigned long long c3 = has ? (r2 & M4[(size_t)v2 * W + lane]) : 0ull;
      const unsigned long long c4 = has ? (r3 & M5[(size_t)v2 * W + lane]) : 0ull;
      if (__ballot(c3 != 0ull) == 0ull || __ballot(c4 != 0ull) == 0ull) continue;
      for (int w3 = 0; w3 < W; ++w3) {
        for (unsigned long long bits3 = word_of(c3, w3); bits3; bits3 &= bits3 - 1ull) {
          const int v3 = w3 * 64 + __builtin_ctzll(bits3);
          unsigned long long x = has ? (c4 & M6[(size_t)v3 * W + lane]) : 0ull;
          if (!FILL) {
            count += (unsigned long long)__popcll(x);
          } else {
            // this lane's quads follow those of the lower lanes (= the lower words)
            const unsigned pc = (unsigned)__popcll(x);
            // the whole wave is here: the block is one wave, and the trip counts, the `continue` above and the return below
            // depend on shuffled words, ballots and `off` alone, which are the same in every lane
            const unsigned incl = wave::scan_incl(pc, lane);
            const unsigned total = __shfl(incl, 63, 64);
            unsigned long long at = off + (incl - pc);
            for (; x && at < cap; x &= x - 1ull, ++at) out[at] = make_int4(v1, v2, v3, lane * 64 + __builtin_ctzll(x));
            off += total;
            if (off >= cap) return;   // (uniform: the base's kept prefix is full)
          }
        }
      }
    }
  }
  if (!FILL) {
    count = wave::sum(count);
    if (lane == 0) row_cnt[(size_t)b * N + v1] = count;
  }
}

// exclusive prefix sums over the N rows of every base: one workgroup per base, a run of rows per thread
__global__ __launch_bounds__(256) void row_starts(const unsigned long long* __restrict__ row_cnt, int N,
                                                  unsigned long long* __restrict__ row_start,
                                                  unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long s_sum[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int per = (N + 255) / 256, lo = min(tid * per, N), hi = min(lo + per, N);
  const unsigned long long* cnt = row_cnt + (size_t)b * N;
  unsigned long long sum = 0ull;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  s_sum[tid] = sum;
  __syncthreads();
  unsigned long long run = 0ull;
  for (int t = 0; t < tid; ++t) run += s_sum[t];
  for (int i = lo; i < hi; ++i) {
    row_start[(size_t)b * N + i] = run;
    run += cnt[i];
  }
  if (tid == 255) totals[b] = run;   // the last thread's running sum is the base's total
}

// picks (base, j) -> the j-th kept quad of that base
__global__ __launch_bounds__(256) void gather_picks(const int4* __restrict__ quads, unsigned long long cap,
                                                    const int2* __restrict__ picks, int m, int4* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  const int2 pk = picks[t];
  out[t] = quads[(size_t)pk.x * cap + (size_t)pk.y];
}

constexpr size_t kMatrixBytes = (size_t)64 << 20;   // the bit matrices of one chunk of bases stay within this
constexpr int kChunkMax = 256;                      // bases per chunk at most (pass A walks them one by one)
constexpr size_t kQuadBytesMax = (size_t)1 << 31;   // resident quads of one batch

}  // namespace

int launch_tetrahedron_bases(pgp_ctx* ctx, unsigned long long seed, int n_attempts, int triangle_trials, int fourth_trials,
                             float max_base_diameter, int* h_ids, float* h_dist, int* h_status, hipStream_t st) {
  if (ctx->nP <= 0 || !ctx->d_P.p) {
    set_error("no scene: call pgp_set_scene first");
    return PGP_ESTATE;
  }
  const size_t A = (size_t)n_attempts;
  Carve c;
  const auto p_ids = c.add<int4>(A, 16);
  const auto p_dist = c.add<float>(6 * A, 16);
  const auto p_status = c.add<int>(A, 16);
  int rc = c.ensure(ctx->d_v4_sel);
  if (rc != PGP_OK) return rc;
  hipLaunchKernelGGL(tetra_bases, dim3((unsigned)n_attempts), dim3(64), 0, st, (const float4*)ctx->d_P.as<float4>(), ctx->nP, seed,
                     triangle_trials, fourth_trials, max_base_diameter, c.at(p_ids), c.at(p_dist), c.at(p_status));
  PGP_HIP(hipGetLastError());
  HostOut out(ctx, st);
  if ((rc = out.to(h_ids, c.at(p_ids), p_ids.bytes())) != PGP_OK || (rc = out.to(h_dist, c.at(p_dist), p_dist.bytes())) != PGP_OK ||
      (rc = out.to(h_status, c.at(p_status), p_status.bytes())) != PGP_OK)
    return rc;
  return out.sync();
}

// The join for nb bases (h_dist[nb][6]): the first min(count, cap) quads of base b go to d_quads[b * cap ...] (ascending), the full
// counts to h_counts[nb].  One synchronisation, at the end.
int launch_v4pcs_join(pgp_ctx* ctx, const float* h_dist, int nb, float eps, long long cap, int4* d_quads, long long* h_counts,
                      hipStream_t st) {
  const int N = ctx->nQs;
  if (N <= 0 || !ctx->d_Qs.p) {
    set_error("no search model: call pgp_set_search_model first");
    return PGP_ESTATE;
  }
  if (N < 4 || N > PGP_V4PCS_MAX_POINTS) {
    set_error("v4pcs: the search model has %d points (4 .. %d)", N, PGP_V4PCS_MAX_POINTS);
    return PGP_EINVAL;
  }
  if (nb == 0) return PGP_OK;
  const int W = (N + 63) / 64;
  const size_t per_base = (size_t)6 * N * W * 8;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>({kMatrixBytes / per_base, (size_t)kChunkMax, (size_t)nb}));
  int rc;
  if ((rc = ctx->d_v4_mat.ensure((size_t)chunk * per_base)) != PGP_OK) return rc;
  Carve c;
  const auto p_dist = c.add<float>((size_t)6 * nb, 16);
  const auto p_tot = c.add<unsigned long long>((size_t)nb, 16);
  const auto p_cnt = c.add<unsigned long long>((size_t)chunk * N, 16);
  const auto p_start = c.add<unsigned long long>((size_t)chunk * N, 16);
  if ((rc = c.ensure(ctx->d_v4_ws)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(c.at(p_dist), h_dist, p_dist.bytes(), hipMemcpyHostToDevice, st));
  unsigned long long* M = ctx->d_v4_mat.as<unsigned long long>();
  const float4* Q = ctx->d_Qs.as<float4>();
  const unsigned grid_a = (unsigned)(((long long)N * W + 3) / 4);
  for (int b0 = 0; b0 < nb; b0 += chunk) {
    const int cb = std::min(chunk, nb - b0);
    hipLaunchKernelGGL(pair_bits, dim3(grid_a), dim3(256), 0, st, Q, N, W, (const float*)(c.at(p_dist) + 6 * (size_t)b0), cb,
                       (double)eps, M);
    hipLaunchKernelGGL(join_rows<false>, dim3((unsigned)(cb * N)), dim3(64), 0, st, (const unsigned long long*)M, N, W, c.at(p_cnt),
                       (const unsigned long long*)nullptr, (int4*)nullptr, 0ull);
    hipLaunchKernelGGL(row_starts, dim3((unsigned)cb), dim3(256), 0, st, (const unsigned long long*)c.at(p_cnt), N, c.at(p_start),
                       c.at(p_tot) + b0);
    if (cap > 0)
      hipLaunchKernelGGL(join_rows<true>, dim3((unsigned)(cb * N)), dim3(64), 0, st, (const unsigned long long*)M, N, W,
                         (unsigned long long*)nullptr, (const unsigned long long*)c.at(p_start), d_quads + (size_t)b0 * (size_t)cap,
                         (unsigned long long)cap);
    PGP_HIP(hipGetLastError());
  }
  static_assert(sizeof(long long) == sizeof(unsigned long long), "");
  PGP_HIP(hipMemcpyAsync(h_counts, c.at(p_tot), p_tot.bytes(), hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

int launch_v4pcs_batch(pgp_ctx* ctx, const float* h_dist, int nb, float eps, int per_base_cap, long long* h_n_quads, int* h_n_stored,
                       hipStream_t st) {
  ctx->v4_nb = 0;   // the resident quads are rewritten below
  ctx->v4_stored.clear();
  if ((size_t)nb * (size_t)per_base_cap * 16 > kQuadBytesMax) {
    set_error("pgp_find_congruent_v4pcs_batch: %d bases x %d quads exceed %zu bytes of resident quads", nb, per_base_cap, kQuadBytesMax);
    return PGP_EINVAL;
  }
  int rc = ctx->d_v4_quads.ensure((size_t)std::max(nb, 1) * (size_t)per_base_cap * 16);
  if (rc != PGP_OK) return rc;
  std::vector<long long> counts((size_t)nb, 0);
  if ((rc = launch_v4pcs_join(ctx, h_dist, nb, eps, per_base_cap, ctx->d_v4_quads.as<int4>(), counts.data(), st)) != PGP_OK) return rc;
  ctx->v4_stored.resize((size_t)nb);
  for (int b = 0; b < nb; ++b) {
    ctx->v4_stored[b] = (int)std::min<long long>(counts[b], per_base_cap);
    if (h_n_quads) h_n_quads[b] = counts[b];
    if (h_n_stored) h_n_stored[b] = ctx->v4_stored[b];
  }
  ctx->v4_nb = nb;
  ctx->v4_cap = per_base_cap;
  return PGP_OK;
}

// picks[m][2] = (base, j) of the resident batch -> d_out[m] (int4); the picks are checked on the host
int launch_v4pcs_gather(pgp_ctx* ctx, const int* h_picks, int m, int4* d_out, hipStream_t st) {
  if (ctx->v4_nb <= 0 || (int)ctx->v4_stored.size() != ctx->v4_nb) {
    set_error("no V4PCS batch: call pgp_find_congruent_v4pcs_batch first (pgp_set_search_model discards it)");
    return PGP_ESTATE;
  }
  for (int k = 0; k < m; ++k) {
    const int b = h_picks[2 * (size_t)k], j = h_picks[2 * (size_t)k + 1];
    if (b < 0 || b >= ctx->v4_nb) {
      set_error("V4PCS batch: pick %d names base %d of %d", k, b, ctx->v4_nb);
      return PGP_EINVAL;
    }
    if (j < 0 || j >= ctx->v4_stored[b]) {
      set_error("V4PCS batch: pick %d names quad %d of the %d kept of base %d", k, j, ctx->v4_stored[b], b);
      return PGP_EINVAL;
    }
  }
  int rc = ctx->d_v4_picks.ensure((size_t)m * 8 + 16);
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(ctx->d_v4_picks.p, h_picks, (size_t)m * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(gather_picks, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const int4*)ctx->d_v4_quads.as<int4>(),
                     (unsigned long long)ctx->v4_cap, (const int2*)ctx->d_v4_picks.as<int2>(), m, d_out);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

}  // namespace pgp
