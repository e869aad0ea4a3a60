// csrc/ppf_vote.hip -- point-pair-feature Hough voting on gfx950: the hypotheses of the node's PPF_HOUGH mode.
//
// SceneCfg::generateHypothesis("PPF_HOUGH") builds pose_candidates::PPFVoting, whose generate
// (PPE/hypothesis_generation/ObjectPoseCandidateSet.cpp:76-117) stops before the estimator.  The reference has no
// estimator to match: this file is the library's statement of Drost et al. (CVPR 2010) over the model's feature table
// of pgp_set_ppf_map (ppf_key.h), restated in numpy by tests/_ppf_restate.py.
//
// Formulas (float arithmetic, every operation rounded on its own: -ffp-contract=off).
//   T_g(p, n)   x -> R_g (x - p).  n^ = n / |n| (|n| == 0: n^ = +x).  When 1 + n^x > 1e-6, with k = 1 / (1 + n^x),
//                 R_g = [[ n^x,  n^y,          n^z        ],
//                        [-n^y,  1 - k n^y^2, -k n^y n^z  ],
//                        [-n^z, -k n^y n^z,    1 - k n^z^2]]
//               (the rotation about n^ x e_x that sends n^ to +x); else R_g = diag(-1, -1, 1).
//   alpha(r, i) q = R_g(p_r, n_r) (p_i - p_r), alpha = atan2f(-q_z, q_y): the rotation about +x that brings q into the
//               half-plane z = 0, y >= 0.
//   alpha_m     of every pair (a, b) of the table's CSR lists, model positions and normals (ppf_alpha_kernel),
//               computed once per (table, model) and kept beside the pair list.
//   vote        reference point s_r = scene point t * ref_step (or an explicit id); for every scene point s_j != s_r
//               with |s_r - s_j|^2 within reach of the table's largest distance key, key = ppf_key(s_r, s_j) (the
//               device function of base selection, unchanged), row = table_find(key); every pair (m_r, m_i) of the
//               row votes +1 into acc[m_r * n_bins + bin], bin = (int)(d * (n_bins / 2 pi)) clamped to n_bins - 1,
//               d = alpha_m - alpha_s, +2 pi when < 0, -2 pi when >= 2 pi.
//   peaks       max over cells of the key (votes << 32 | ~cell): most votes, then the lowest cell; further peaks take
//               the maximum below the previous key.  Kept while votes > 0, votes >= min_votes and
//               (float)votes >= min_vote_fraction * (float)first.
//   pose        T = T_s^-1 R_x(alpha) T_m, alpha = (bin + 0.5) * (2 pi / n_bins) (float), R_x(a) = [[1,0,0],[0,c,-s],
//               [0,s,c]]: rotation R_s^T (R_x R_m), translation R_s^T (R_x (-R_m p_m)) + p_s, written column-major.
//
// Mapping.
//   ppf_vote_kernel<kLds>  512 threads per workgroup, workgroups walk the reference points t = blockIdx.x,
//                          + gridDim.x, ...; a lane per scene point j computes the key and probes the hash set; the
//                          wave then walks the pairs of its 64 rows as one list (a prefix sum of the row lengths in
//                          LDS, a 6-step search per pair: every lane busy and consecutive pairs coalesced, although
//                          row lengths differ by orders of magnitude) and votes with integer atomics into the
//                          accumulator: in LDS when n_model x n_bins x 4 + 6 KiB fits 152 KiB, else in an HBM slice per
//                          workgroup (a slice per reference point in flight; read back with agent-scope loads).  Counts
//                          do not depend on the order of arrival: bitwise reproducible.  The peaks are block-wide
//                          64-bit max reductions of the packed key, one per kept peak.
//   ppf_emit_kernel        one workgroup: ballot + prefix over the (reference, peak) slots in order, the pose of
//                          every kept slot, the full count.

#include "pgp_internal.h"
#include "wave.h"
#include "ppf_key.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace pgp {

using namespace ppfk;

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kEmitThreads = 1024;
constexpr size_t kLdsBudget = 160 * 1024 - 8 * 1024;
constexpr float kTwoPi = 6.28318530717958647692f;
constexpr int kStage = 192;   // ints of LDS per wave: the rows of its 64 scene points
constexpr size_t kFixedLds = kWaves * 8 + kWaves * kStage * 4;   // peak reduction + row staging

struct Frame {
  float r[9];   // R_g, row-major
  V3 p;
};

__host__ __device__ inline Frame frame_of(V3 p, V3 n) {
  Frame f;
  f.p = p;
  const float l = sqrtf(n.x * n.x + n.y * n.y + n.z * n.z);
  float nx = 1.f, ny = 0.f, nz = 0.f;
  if (l > 0.f) {
    nx = n.x / l;
    ny = n.y / l;
    nz = n.z / l;
  }
  if (1.f + nx > 1e-6f) {
    const float k = 1.f / (1.f + nx);
    f.r[0] = nx;
    f.r[1] = ny;
    f.r[2] = nz;
    f.r[3] = -ny;
    f.r[4] = 1.f - k * ny * ny;
    f.r[5] = -(k * ny * nz);
    f.r[6] = -nz;
    f.r[7] = -(k * ny * nz);
    f.r[8] = 1.f - k * nz * nz;
  } else {
    f.r[0] = -1.f;
    f.r[1] = 0.f;
    f.r[2] = 0.f;
    f.r[3] = 0.f;
    f.r[4] = -1.f;
    f.r[5] = 0.f;
    f.r[6] = 0.f;
    f.r[7] = 0.f;
    f.r[8] = 1.f;
  }
  return f;
}

__device__ __forceinline__ float alpha_of(const Frame& f, V3 x) {
  const float dx = x.x - f.p.x, dy = x.y - f.p.y, dz = x.z - f.p.z;
  const float qy = f.r[3] * dx + f.r[4] * dy + f.r[5] * dz;
  const float qz = f.r[6] * dx + f.r[7] * dy + f.r[8] * dz;
  return atan2f(-qz, qy);
}

__device__ __forceinline__ int alpha_bin(float d, float scale, int n_bins) {
  if (d < 0.f) d += kTwoPi;
  else if (d >= kTwoPi) d -= kTwoPi;
  const int b = (int)(d * scale);
  return b < 0 ? 0 : (b >= n_bins ? n_bins - 1 : b);
}

__device__ __forceinline__ V3 v3(float4 v) { return {v.x, v.y, v.z}; }

__global__ __launch_bounds__(256) void ppf_alpha_kernel(const float4* __restrict__ M, const float4* __restrict__ Mn, int n,
                                                        const int2* __restrict__ pairs, long long n_pairs,
                                                        float* __restrict__ alpha) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_pairs) return;
  const int2 pr = pairs[k];
  if ((unsigned)pr.x >= (unsigned)n || (unsigned)pr.y >= (unsigned)n) {   // excluded by the host checks
    alpha[k] = 0.f;
    return;
  }
  alpha[k] = alpha_of(frame_of(v3(M[pr.x]), v3(Mn[pr.x])), v3(M[pr.y]));
}

struct VoteArgs {
  const float4* P;     // {x, y, z, id}
  const float4* Pnw;   // {nx, ny, nz, w}
  int nP;
  const float4* M;     // PPF model positions
  const float4* Mn;    // its normals
  int n_model;
  PpfTable tab;
  const uint32_t* off;   // CSR offsets per table row
  const int2* pairs;
  const float* alpha;    // alpha_m per pair
  float skip2;           // |u|^2 beyond which no key of the table can match
  const int* ref_ids;    // nullable: explicit reference points
  int n_ref, step;
  int n_bins;
  float bin_scale;       // n_bins / 2 pi
  int ppr;
  float min_frac;
  int min_votes;
  int* hbm_acc;          // HBM path: one slice of n_model * n_bins counters per workgroup
  int* acc_out;          // nullable: [n_ref][n_model * n_bins]
  int2* slots;           // [n_ref * ppr] {votes (0: none), cell}
};

template <bool kLds>
__device__ __forceinline__ int load_acc(const int* p) {
  if (kLds) return *p;
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past the CU's vector cache
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void ppf_vote_kernel(VoteArgs a) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  const int cells = a.n_model * a.n_bins;
  int* acc = kLds ? smem : a.hbm_acc + (size_t)blockIdx.x * cells;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(smem + (kLds ? ((cells + 3) & ~3) : 0));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* w_pref = reinterpret_cast<int*>(red + kWaves) + wave * kStage;   // the wave's rows: inclusive ends,
  int* w_base = w_pref + 64;                                            // first pair - exclusive start,
  float* w_as = reinterpret_cast<float*>(w_pref + 128);                 // alpha_s
  for (int t = blockIdx.x; t < a.n_ref; t += gridDim.x) {
    for (int c = tid; c < cells; c += kThreads) acc[c] = 0;
    __syncthreads();
    const int r = a.ref_ids ? a.ref_ids[t] : t * a.step;
    const V3 pr = ld3(a.P, r), nr = v3(a.Pnw[r]);
    const Frame fr = frame_of(pr, nr);
    for (int j0 = wave * 64; j0 < a.nP; j0 += kThreads) {   // wave-uniform trip count
      const int j = j0 + lane;
      int cnt = 0, first = 0;
      float as = 0.f;
      if (j < a.nP && j != r) {
        const V3 pj = ld3(a.P, j);
        const V3 u = vsub(pr, pj);
        if (sqnorm_eigen(u) <= a.skip2) {
          const int row = table_find(a.tab, ppf_key(a.tab, pr, nr, pj, v3(a.Pnw[j]), nullptr));
          if (row >= 0) {
            first = (int)a.off[row];
            cnt = (int)a.off[row + 1] - first;
            as = alpha_of(fr, pj);
          }
        }
      }
      // the wave's rows are walked as ONE list, 64 consecutive pairs per step (row lengths vary by orders of magnitude)
      const int inc = wave::scan_incl(cnt, lane);
      const int total = __shfl(inc, 63);
      if (total == 0) continue;
      w_pref[lane] = inc;
      w_base[lane] = first - (inc - cnt);
      w_as[lane] = as;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int e = lane; e < total; e += 64) {
        int src = 0;   // the first lane whose rows end beyond e
#pragma unroll
        for (int b = 32; b >= 1; b >>= 1)
          if (w_pref[src + b - 1] <= e) src += b;
        const int k = w_base[src] + e;
        const int mr = a.pairs[k].x;
        if ((unsigned)mr < (unsigned)a.n_model)
          atomicAdd(&acc[mr * a.n_bins + alpha_bin(a.alpha[k] - w_as[src], a.bin_scale, a.n_bins)], 1);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // before the next trip rewrites the staging
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    if (a.acc_out)
      for (int c = tid; c < cells; c += kThreads) a.acc_out[(size_t)t * cells + c] = load_acc<kLds>(acc + c);
    unsigned long long prev = ~0ull;
    int first = 0;
    bool go = true;
    for (int p = 0; p < a.ppr; ++p) {
      unsigned long long best = 0;
      if (go) {   // uniform over the workgroup
        for (int c = tid; c < cells; c += kThreads) {
          const unsigned long long key =
              ((unsigned long long)(unsigned)load_acc<kLds>(acc + c) << 32) | (0xFFFFFFFFu - (unsigned)c);
          if (key < prev && key > best) best = key;
        }
        best = wave::max(best);
        if (lane == 0) red[wave] = best;
        __syncthreads();
        best = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) best = red[w] > best ? red[w] : best;
        __syncthreads();
      }
      const int v = (int)(best >> 32), cell = (int)(0xFFFFFFFFu - (unsigned)best);
      if (p == 0) first = v;
      const bool ok = go && v > 0 && v >= a.min_votes && (float)v >= a.min_frac * (float)first;
      if (tid == 0) a.slots[(size_t)t * a.ppr + p] = make_int2(ok ? v : 0, ok ? cell : -1);
      go = ok;
      prev = best;
    }
    __syncthreads();   // before the next reference point clears the accumulator
  }
}

struct EmitArgs {
  const int2* slots;
  int n_slots, ppr;
  const int* ref_ids;
  int step;
  const float4* P;
  const float4* Pnw;
  const float4* M;
  const float4* Mn;
  int n_bins;
  float* T;
  int* votes;
  int* ref;
  int* cell;
  float* scores;   // nullable: zeroed pads
  int cap;
  int* n_out;
  int pad_to;      // entries [n_out, pad_to) of T receive NaN transforms (they score 0), votes 0
};

__device__ void pose_of(V3 ps, V3 ns, V3 pm, V3 nm, float alpha, float* __restrict__ T) {
  const Frame fs = frame_of(ps, ns), fm = frame_of(pm, nm);
  const float c = cosf(alpha), s = sinf(alpha);
  float A[9];   // R_x R_m
  for (int j = 0; j < 3; ++j) {
    A[j] = fm.r[j];
    A[3 + j] = c * fm.r[3 + j] - s * fm.r[6 + j];
    A[6 + j] = s * fm.r[3 + j] + c * fm.r[6 + j];
  }
  const float tm0 = -(fm.r[0] * pm.x + fm.r[1] * pm.y + fm.r[2] * pm.z);
  const float tm1 = -(fm.r[3] * pm.x + fm.r[4] * pm.y + fm.r[5] * pm.z);
  const float tm2 = -(fm.r[6] * pm.x + fm.r[7] * pm.y + fm.r[8] * pm.z);
  const float w[3] = {tm0, c * tm1 - s * tm2, s * tm1 + c * tm2};
  const float p[3] = {ps.x, ps.y, ps.z};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * j + i] = fs.r[i] * A[j] + fs.r[3 + i] * A[3 + j] + fs.r[6 + i] * A[6 + j];
    T[12 + i] = (fs.r[i] * w[0] + fs.r[3 + i] * w[1] + fs.r[6 + i] * w[2]) + p[i];
    T[4 * i + 3] = 0.f;
  }
  T[15] = 1.f;
}

__global__ __launch_bounds__(kEmitThreads) void ppf_emit_kernel(EmitArgs a) {
  __shared__ int wsum[kEmitThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < a.n_slots; base += kEmitThreads) {
    const int i = base + tid;
    const int2 s = i < a.n_slots ? a.slots[i] : make_int2(0, -1);
    const bool v = s.x > 0;
    const unsigned long long m = __ballot(v);
    const int rank = wave::rank_in(m, lane);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int q = 0; q < kEmitThreads / 64; ++q) {
      const int cnt = wsum[q];
      before += q < wave ? cnt : 0;
      total += cnt;
    }
    const int idx = carry + before + rank;
    if (v && idx < a.cap) {
      const int t = i / a.ppr;
      const int r = a.ref_ids ? a.ref_ids[t] : t * a.step;
      const int mr = s.y / a.n_bins, bin = s.y - mr * a.n_bins;
      const float alpha = ((float)bin + 0.5f) * (kTwoPi / (float)a.n_bins);
      pose_of(ld3(a.P, r), v3(a.Pnw[r]), v3(a.M[mr]), v3(a.Mn[mr]), alpha, a.T + (size_t)idx * 16);
      a.votes[idx] = s.x;
      if (a.ref) a.ref[idx] = r;
      if (a.cell) a.cell[idx] = s.y;
    }
    carry += total;
    __syncthreads();
  }
  if (tid == 0) *a.n_out = carry;
  for (int idx = carry + tid; idx < a.pad_to && idx < a.cap; idx += kEmitThreads) {
    for (int e = 0; e < 16; ++e) a.T[(size_t)idx * 16 + e] = __int_as_float(0x7FC00000);
    a.votes[idx] = 0;
    if (a.scores) a.scores[idx] = 0.f;
  }
}

bool force_hbm() {
  const char* e = getenv("PGP_PPF_ACC");
  return e && std::strcmp(e, "hbm") == 0;
}

}  // namespace

int ppf_model_angles(pgp_ctx* ctx) {
  ctx->ppf_alpha_ready = false;
  if (!ctx->ppf_ready || !ctx->ppf_has_pairs || ctx->ppf_model_n < 0) return PGP_OK;
  if (ctx->ppf_n_pairs > 0 && (ctx->ppf_id_min < 0 || ctx->ppf_id_max >= ctx->ppf_model_n)) return PGP_OK;   // EINVAL at the vote
  const long long np = ctx->ppf_n_pairs;
  int rc = ctx->d_ppf_alpha.ensure((size_t)std::max(np, 1LL) * 4);
  if (rc != PGP_OK) return rc;
  if (np > 0) {
    const int n = ctx->ppf_model_n;
    const float4* M = ctx->d_ppf_model.as<float4>();
    hipLaunchKernelGGL(ppf_alpha_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, M,
                       M + n, n, ctx->d_ppf_pairs.as<int2>(), np, ctx->d_ppf_alpha.as<float>());
    PGP_HIP(hipGetLastError());
    PGP_HIP(hipStreamSynchronize(ctx->stream));
  }
  ctx->ppf_alpha_ready = true;
  return PGP_OK;
}

int ppf_vote_check(pgp_ctx* ctx, const pgp_ppf_options* o, const char* who) {
  if (!o || o->ref_step < 1 || o->n_bins < 1 || o->n_bins > 360 || o->peaks_per_ref < 1 || o->peaks_per_ref > 4 ||
      !(o->min_vote_fraction >= 0.f && o->min_vote_fraction <= 1.f) || o->min_votes < 1) {
    set_error("%s: bad options (ref_step >= 1, 1 <= n_bins <= 360, 1 <= peaks_per_ref <= 4, "
              "0 <= min_vote_fraction <= 1, min_votes >= 1)", who);
    return PGP_EINVAL;
  }
  if (!ctx->has_scene_normals) {
    set_error("%s: needs a scene with normals: call pgp_set_scene first", who);
    return PGP_ESTATE;
  }
  if (!ctx->ppf_ready || !ctx->ppf_has_pairs) {
    set_error("%s: no pair-feature table with pair lists: call pgp_set_ppf_map with pairs first", who);
    return PGP_ESTATE;
  }
  if (ctx->ppf_model_n < 0) {
    set_error("%s: no PPF model: call pgp_set_ppf_model first", who);
    return PGP_ESTATE;
  }
  if (ctx->ppf_n_pairs > 0 && (ctx->ppf_id_min < 0 || ctx->ppf_id_max >= ctx->ppf_model_n)) {
    set_error("%s: the PPF model has %d points, the table's pair ids span [%d, %d]", who, ctx->ppf_model_n,
              ctx->ppf_id_min, ctx->ppf_id_max);
    return PGP_EINVAL;
  }
  if ((long long)ctx->ppf_model_n * o->n_bins > INT_MAX / 2) {
    set_error("%s: n_model x n_bins = %lld cells is too many", who, (long long)ctx->ppf_model_n * o->n_bins);
    return PGP_EINVAL;
  }
  if (!ctx->ppf_alpha_ready) {
    set_error("%s: the model angles are missing (a failed pgp_set_ppf_model / pgp_set_ppf_map?)", who);
    return PGP_ESTATE;
  }
  return PGP_OK;
}

int ppf_slots(const pgp_ctx* ctx, const pgp_ppf_options* o) {
  if (ctx->nP <= 0 || ctx->ppf_model_n <= 0) return 0;
  return ((ctx->nP - 1) / o->ref_step + 1) * o->peaks_per_ref;
}

int launch_ppf_vote(pgp_ctx* ctx, const pgp_ppf_options* o, const int* d_ref_ids, int n_ref_ids, int* d_acc_out, float* d_T,
                    int* d_votes, int* d_ref, int* d_cell, int cap, int* d_n_out, int pad_to, hipStream_t st) {
  const int nP = ctx->nP, n_model = ctx->ppf_model_n;
  const int n_ref = d_ref_ids ? n_ref_ids : (nP > 0 ? (nP - 1) / o->ref_step + 1 : 0);
  const int cells = n_model * o->n_bins;
  if (n_ref == 0 || cells == 0 || ctx->ppf_n_pairs == 0 || ctx->ppf_max_f1 < 0) {
    if (d_acc_out && n_ref > 0 && cells > 0) PGP_HIP(hipMemsetAsync(d_acc_out, 0, (size_t)n_ref * cells * 4, st));
    PGP_HIP(hipMemsetAsync(d_n_out, 0, 4, st));
    if (pad_to > 0) {   // nothing voted: every pad is a NaN transform
      EmitArgs e{};
      e.n_slots = 0;
      e.ppr = 1;
      e.n_bins = 1;
      e.T = d_T;
      e.votes = d_votes;
      e.cap = cap;
      e.n_out = d_n_out;
      e.pad_to = pad_to;
      hipLaunchKernelGGL(ppf_emit_kernel, dim3(1), dim3(kEmitThreads), 0, st, e);
      PGP_HIP(hipGetLastError());
    }
    return PGP_OK;
  }
  int rc = await_index(ctx, st);   // the scene's uploads are through once its index build is
  if (rc != PGP_OK) return rc;
  const size_t lds = (((size_t)cells + 3) & ~(size_t)3) * 4 + kFixedLds;
  const bool in_lds = lds <= kLdsBudget && !force_hbm();
  int n_cu = 0;
  PGP_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int grid = in_lds ? std::min(n_ref, 65535) : std::min(n_ref, std::max(n_cu, 1));
  const size_t n_slots = (size_t)n_ref * o->peaks_per_ref;
  const size_t b_slots = (n_slots * 8 + 255) & ~(size_t)255;
  const size_t b_acc = in_lds ? 0 : (size_t)grid * cells * 4;
  if ((rc = ctx->d_ppf_ws.ensure(b_slots + b_acc)) != PGP_OK) return rc;
  unsigned char* ws = ctx->d_ppf_ws.as<unsigned char>();
  const float4* M = ctx->d_ppf_model.as<float4>();
  VoteArgs a{};
  a.P = ctx->d_P.as<float4>();
  a.Pnw = ctx->d_Pnw.as<float4>();
  a.nP = nP;
  a.M = M;
  a.Mn = M + n_model;
  a.n_model = n_model;
  fill_ppf_table(ctx, &a.tab);
  a.off = ctx->d_ppf_off.as<uint32_t>();
  a.pairs = ctx->d_ppf_pairs.as<int2>();
  a.alpha = ctx->d_ppf_alpha.as<float>();
  // f1 = approximate_bin((int)(|u| * 1000), 5) <= max_f1 needs |u| * 1000 < max_f1 + 5: 1 % of slack for the float steps
  const float reach = (float)(ctx->ppf_max_f1 + 5) * 1e-3f * 1.01f;
  a.skip2 = reach * reach;
  a.ref_ids = d_ref_ids;
  a.n_ref = n_ref;
  a.step = o->ref_step;
  a.n_bins = o->n_bins;
  a.bin_scale = (float)o->n_bins / kTwoPi;
  a.ppr = o->peaks_per_ref;
  a.min_frac = o->min_vote_fraction;
  a.min_votes = o->min_votes;
  a.hbm_acc = in_lds ? nullptr : reinterpret_cast<int*>(ws + b_slots);
  a.acc_out = d_acc_out;
  a.slots = reinterpret_cast<int2*>(ws);
  if (in_lds) {
    if (lds > 64 * 1024)
      PGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ppf_vote_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ppf_vote_kernel<true>, dim3(grid), dim3(kThreads), lds, st, a);
  } else {
    hipLaunchKernelGGL(ppf_vote_kernel<false>, dim3(grid), dim3(kThreads), kFixedLds, st, a);
  }
  PGP_HIP(hipGetLastError());
  EmitArgs e{};
  e.slots = a.slots;
  e.n_slots = (int)n_slots;
  e.ppr = o->peaks_per_ref;
  e.ref_ids = d_ref_ids;
  e.step = o->ref_step;
  e.P = a.P;
  e.Pnw = a.Pnw;
  e.M = a.M;
  e.Mn = a.Mn;
  e.n_bins = o->n_bins;
  e.T = d_T;
  e.votes = d_votes;
  e.ref = d_ref;
  e.cell = d_cell;
  e.cap = cap;
  e.n_out = d_n_out;
  e.pad_to = pad_to;
  hipLaunchKernelGGL(ppf_emit_kernel, dim3(1), dim3(kEmitThreads), 0, st, e);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

}  // namespace pgp
