// csrc/tricp_states.hip -- trimmed-ICP refinement of MCTS child states, ONE WORKGROUP PER STATE.
//
// Replaces UCTState::performTrICP (PPE/hypothesis_verification/mcts/UCTState.cpp:137-139, 142-174, 194), which
// UCTSearch.cpp:98, 157, 225 call between updateNewObject and correctPhysics: the newest object's segment, minus the
// points its already placed neighbours explain, is aligned onto the object's model by pcl::recognition::TrimmedICP.
// PCL is not in the reference tree, so the ICP is the library's own definition (the header of csrc/icp.hip, restated
// by tests/_icp_restate.py); the whole chain is restated by tests/_tricp_restate.py.
//
// A level of the search holds up to 256 states, each with its own unexplained subset of its object's segment -- its
// own source cloud and its own trimmed count -- which is the opposite shape of pgp_icp_refine (one source cloud, n
// guesses).  So a workgroup of 256 threads (four waves: the block4_* helpers of wave.h) owns a state from the filter to
// the final pose.  Workgroups do not communicate, nothing spins or waits, every loop is bounded by a count known at
// launch (segment and model sizes, 16 statics, max_iterations <= 1000): a state's result cannot depend on its
// neighbours in the batch.  Per state:
//   1. read the object index o, the pose T (object -> camera) and the statics (object, pose), at most 16;
//   2. unexplained filter (skipped without statics or with r <= 0): a segment point is dropped when any point of any
//      static's OWN model, placed ((g0 x + g1 y) + g2 z) + t, has d2 = (dx^2 + dy^2) + dz^2 < r * r (float32 product):
//      explained_points' arithmetic (preprocess.hip).  The kept points are compacted in their original order
//      (block4_rank) and live in LDS only;
//   3. G = rigid inverse of T as select.hip's top_gather forms it: {R^T, -R^T t} in double, rounded once;
//   4. TrimmedICP of the kept points onto the object's model: placement by row_xf, d2 = dx^2 + (dy^2 + dz^2), nearest =
//      smallest d2 then lowest target index by a tiled exhaustive scan (the model goes through a 1024-point LDS tile
//      read as broadcasts, up to four placed points per lane in registers), k = (int)|trim * (float)n_kept| clamped to
//      [1, n_kept], the k smallest d2 by an exact radix select on the float bits with ties by lowest source index
//      (ordered scan), float64 sums in a fixed tree (thread t adds the points 4 t .. 4 t + 3 of every 1024 in index
//      order, then sum_dpp(double), then block4_total's order over the waves), solve_rigid in one lane; repeated while
//      E / E_old < energy_ratio and iterations < max_iterations.  A point with no neighbour below FLT_MAX keeps
//      d2 = FLT_MAX, may be ranked by the trim and never enters a sum;
//   5. T <- rigid inverse of G by the same rule; energy, iters, n_kept.
// The library's own rules: k < 3 leaves the state as it came (T is not written, iters = 0, energy = 0); a non-finite
// pose, an unknown object index (the state's or a static's), a static range outside 0 .. 16 or a segment beyond the
// launch's LDS capacity gives a NaN T, iters = -1, energy = 0, n_kept = 0.
//
// LDS: a fixed part (tile 16 KB, sums, histogram) and 18 bytes per segment point (x, y, z, d2 as float, the
// correspondence as 16 bits: models hold at most 65535 points, 0xFFFF = none), sized from the LARGEST segment of the
// resident set: 300-point segments take 27 KB and leave room for five workgroups per CU, 4096-point ones 90 KB.
// No float atomics (the histogram's are integer LDS atomics), no HBM scratch per state.

#include "pgp_internal.h"
#include "wave.h"
#include "icp_solve.h"

#include <cfloat>
#include <cmath>

namespace pgp {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;        // model points per LDS tile
constexpr int kSweep = 4;          // segment points per lane per sweep: a sweep covers kSweep * kThreads points
constexpr int kNSum = 17;          // solve_rigid's 16 sums + the energy

struct alignas(16) TricpLds {
  float4 tile[kTile];
  double red[4][kNSum];
  double sum[kNSum];
  double e_old;
  float G[16];
  unsigned hist[256];
  unsigned cnt[4];
  unsigned prefix, kleft, sel_bin, sel_acc, carry;
  int go;
};
static_assert(sizeof(TricpLds) % 16 == 0, "the per-point arrays behind it stay 16-byte aligned");

struct TricpArgs {
  const TricpObject* objs;
  int n_obj;
  int n_states;
  const int* obj;      // nullable: obj_uniform
  int obj_uniform;
  float* T;            // [n_states][16] in/out
  const int* soff;     // [n_states + 1]
  const int* sobj;     // nullable: static j of a state is object j - soff[state]
  const float* sT;
  float trim, r2, ratio;
  int filter;          // removal_radius > 0
  int max_iter;
  float* energy;       // nullable
  int* iters;          // nullable
  int* n_kept;         // nullable
  int cap;             // segment points the launch's LDS holds (a multiple of kThreads)
};

// rigid inverse of a column-major 4x4, select.hip top_gather's rule: double, rounded once
__device__ __forceinline__ void rigid_inverse(const float* m, float* o) {
  const double tx = m[12], ty = m[13], tz = m[14];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = m[4 * r], b = m[4 * r + 1], c = m[4 * r + 2];
    o[r] = (float)a;
    o[4 + r] = (float)b;
    o[8 + r] = (float)c;
    o[12 + r] = (float)(-(a * tx + b * ty + c * tz));
  }
  o[3] = o[7] = o[11] = 0.f;
  o[15] = 1.f;
}

// Unexplained filter of the segment points base + r * 256 + tid, r < R, against every static of the state, and their
// ordered compaction to sx/sy/sz[carry ..]; returns the new carry.  Called by the whole block.
template <int R>
__device__ __forceinline__ unsigned filter_sweep(TricpLds& L, const TricpArgs& a, float* sx, float* sy, float* sz, int base,
                                                 int n_seg, int s0, int ns, unsigned carry) {
  const int tid = threadIdx.x, lane = tid & 63;
  float x[R], y[R], z[R];
  bool hit[R], in[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = base + r * kThreads + tid;
    in[r] = i < n_seg;
    x[r] = in[r] ? sx[i] : 0.f;
    y[r] = in[r] ? sy[i] : 0.f;
    z[r] = in[r] ? sz[i] : 0.f;
    hit[r] = false;
  }
  for (int s = 0; s < ns; ++s) {
    const int os = a.sobj ? a.sobj[s0 + s] : s;
    const TricpObject ob = a.objs[os];
    const float* G = a.sT + 16 * (size_t)(s0 + s);
    const float g0 = G[0], g1 = G[1], g2 = G[2], g4 = G[4], g5 = G[5], g6 = G[6], g8 = G[8], g9 = G[9], g10 = G[10],
                g12 = G[12], g13 = G[13], g14 = G[14];
    for (int t0 = 0; t0 < ob.n_model; t0 += kTile) {
      const int tn = min(kTile, ob.n_model - t0);
      __syncthreads();   // the previous tile is consumed
      for (int j = tid; j < tn; j += kThreads) {
        const float4 p = ob.model[t0 + j];
        L.tile[j] = make_float4(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g0, p.x), __fmul_rn(g4, p.y)), __fmul_rn(g8, p.z)), g12),
                                __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g1, p.x), __fmul_rn(g5, p.y)), __fmul_rn(g9, p.z)), g13),
                                __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g2, p.x), __fmul_rn(g6, p.y)), __fmul_rn(g10, p.z)), g14), 0.f);
      }
      __syncthreads();
      bool alive = false;
#pragma unroll
      for (int r = 0; r < R; ++r) alive |= in[r] && !hit[r];
      if (__ballot(alive) != 0ull) {   // a wave whose points are all explained only keeps the barriers
#pragma unroll 8   // a workgroup has ONE wave per SIMD: the tile reads have to be in flight ahead of the arithmetic
        for (int j = 0; j < tn; ++j) {
          const float4 m = L.tile[j];   // broadcast read
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float dx = __fsub_rn(x[r], m.x), dy = __fsub_rn(y[r], m.y), dz = __fsub_rn(z[r], m.z);
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            hit[r] |= d2 < a.r2;
          }
        }
      }
    }
  }
  __syncthreads();   // every thread holds its points: the compaction may overwrite them
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool keep = in[r] && !hit[r];
    const unsigned long long ballot = __ballot(keep);
    wave::block4_publish(L.cnt, lane == 0, (unsigned)__popcll(ballot));
    const unsigned dst = wave::block4_rank(L.cnt, ballot, carry);   // <= base + r * 256 + tid
    if (keep) {
      sx[dst] = x[r];
      sy[dst] = y[r];
      sz[dst] = z[r];
    }
    carry += wave::block4_total(L.cnt);
    __syncthreads();   // L.cnt is free again
  }
  return carry;
}

// Nearest model point of the kept points base + r * 256 + tid, r < R, placed by L.G.  Called by the whole block.
template <int R>
__device__ __forceinline__ void nn_sweep(TricpLds& L, const float* sx, const float* sy, const float* sz, float* d2o,
                                         unsigned short* jo, int base, int n_kept, const float4* __restrict__ model, int n_model) {
  const int tid = threadIdx.x;
  const float g00 = L.G[0], g10 = L.G[1], g20 = L.G[2], g01 = L.G[4], g11 = L.G[5], g21 = L.G[6], g02 = L.G[8], g12 = L.G[9],
              g22 = L.G[10], g03 = L.G[12], g13 = L.G[13], g23 = L.G[14];
  float x[R], y[R], z[R], best[R];
  int bj[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = base + r * kThreads + tid;
    const bool in = i < n_kept;
    const float px = in ? sx[i] : 0.f, py = in ? sy[i] : 0.f, pz = in ? sz[i] : 0.f;
    x[r] = row_xf(g00, g01, g02, g03, px, py, pz);
    y[r] = row_xf(g10, g11, g12, g13, px, py, pz);
    z[r] = row_xf(g20, g21, g22, g23, px, py, pz);
    best[r] = FLT_MAX;
    bj[r] = -1;
  }
  for (int t0 = 0; t0 < n_model; t0 += kTile) {
    const int tn = min(kTile, n_model - t0);
    __syncthreads();   // the previous tile is consumed
    for (int j = tid; j < tn; j += kThreads) L.tile[j] = model[t0 + j];
    __syncthreads();
#pragma unroll 8   // one wave per SIMD: nothing else hides the tile reads' latency
    for (int j = 0; j < tn; ++j) {
      const float4 m = L.tile[j];   // broadcast read
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float dx = __fsub_rn(x[r], m.x), dy = __fsub_rn(y[r], m.y), dz = __fsub_rn(z[r], m.z);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fadd_rn(__fmul_rn(dy, dy), __fmul_rn(dz, dz)));
        if (d2 < best[r]) {   // strict: the lowest j wins ties
          best[r] = d2;
          bj[r] = t0 + j;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = base + r * kThreads + tid;
    if (i < n_kept) {
      d2o[i] = best[r];
      jo[i] = (unsigned short)(bj[r] < 0 ? 0xFFFF : bj[r]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void tricp_states(TricpArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  TricpLds& L = *reinterpret_cast<TricpLds*>(smem);
  float* sx = reinterpret_cast<float*>(smem + sizeof(TricpLds));
  float* sy = sx + a.cap;
  float* sz = sy + a.cap;
  float* sd2 = sz + a.cap;
  unsigned short* sj = reinterpret_cast<unsigned short*>(sd2 + a.cap);

  const int state = blockIdx.x;
  if (state >= a.n_states) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* Tg = a.T + 16 * (size_t)state;

  // ---- 1. the state, checked (every thread reads the same words: the verdict is uniform) ----
  const int o = a.obj ? a.obj[state] : a.obj_uniform;
  const int s0 = a.soff[state], ns = a.soff[state + 1] - s0;
  bool bad = o < 0 || o >= a.n_obj || ns < 0 || ns > PGP_TRICP_MAX_STATICS || s0 < 0;
  if (!bad && a.sobj)
    for (int s = 0; s < ns; ++s) {
      const int os = a.sobj[s0 + s];
      bad |= os < 0 || os >= a.n_obj;
    }
  if (!bad && !a.sobj) bad = ns > a.n_obj;
  if (!a.sT) bad |= ns != 0;   // the caller passed no static poses: no state may have statics
  float Tin[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    Tin[q] = Tg[q];
    bad |= !isfinite(Tin[q]);
  }
  TricpObject ob{nullptr, nullptr, 0, 0};
  if (!bad) {
    ob = a.objs[o];
    bad = ob.n_seg > a.cap;
  }
  if (bad) {
    if (tid < 16) Tg[tid] = __int_as_float(0x7FC00000);
    if (tid == 0) {
      if (a.energy) a.energy[state] = 0.f;
      if (a.iters) a.iters[state] = -1;
      if (a.n_kept) a.n_kept[state] = 0;
    }
    return;
  }

  // ---- 2. the segment into LDS, the unexplained filter, the ordered compaction ----
  const int n_seg = ob.n_seg;
  for (int i = tid; i < n_seg; i += kThreads) {
    const float4 p = ob.seg[i];
    sx[i] = p.x;
    sy[i] = p.y;
    sz[i] = p.z;
  }
  __syncthreads();
  int n_kept = n_seg;
  if (a.filter && ns > 0) {
    unsigned carry = 0;
    for (int base = 0; base < n_seg; base += kSweep * kThreads) {
      const int rows = min(kSweep, (n_seg - base + kThreads - 1) / kThreads);   // uniform
      if (rows == 1) carry = filter_sweep<1>(L, a, sx, sy, sz, base, n_seg, s0, ns, carry);
      else if (rows == 2) carry = filter_sweep<2>(L, a, sx, sy, sz, base, n_seg, s0, ns, carry);
      else if (rows == 3) carry = filter_sweep<3>(L, a, sx, sy, sz, base, n_seg, s0, ns, carry);
      else carry = filter_sweep<4>(L, a, sx, sy, sz, base, n_seg, s0, ns, carry);
    }
    n_kept = (int)carry;
  }

  // ---- the trimmed count; fewer than three pairs: the state stays as it came ----
  int k = (int)fabsf(__fmul_rn(a.trim, (float)n_kept));
  k = min(max(k, 1), n_kept);
  if (k < 3) {
    if (tid == 0) {
      if (a.energy) a.energy[state] = 0.f;
      if (a.iters) a.iters[state] = 0;
      if (a.n_kept) a.n_kept[state] = n_kept;
    }
    return;
  }

  // ---- 3. the guess ----
  if (tid == 0) {
    rigid_inverse(Tin, L.G);
    L.e_old = (double)FLT_MAX;   // PCL: the energy starts at numeric_limits<float>::max()
  }
  __syncthreads();

  // ---- 4. trimmed ICP ----
  int it = 0;
  float e_last = 0.f;
  while (it < a.max_iter) {
    // correspondences
    for (int base = 0; base < n_kept; base += kSweep * kThreads) {
      const int rows = min(kSweep, (n_kept - base + kThreads - 1) / kThreads);   // uniform
      if (rows == 1) nn_sweep<1>(L, sx, sy, sz, sd2, sj, base, n_kept, ob.model, ob.n_model);
      else if (rows == 2) nn_sweep<2>(L, sx, sy, sz, sd2, sj, base, n_kept, ob.model, ob.n_model);
      else if (rows == 3) nn_sweep<3>(L, sx, sy, sz, sd2, sj, base, n_kept, ob.model, ob.n_model);
      else nn_sweep<4>(L, sx, sy, sz, sd2, sj, base, n_kept, ob.model, ob.n_model);
    }
    __syncthreads();

    // the k-th smallest d2 by radix select on the float bits (d2 >= 0: the bits order as the values)
    unsigned thr_key = 0xFFFFFFFFu, ties_to_take = 0xFFFFFFFFu;   // k == n_kept: everything
    if (k < n_kept) {
      if (tid == 0) {
        L.prefix = 0;
        L.kleft = (unsigned)k;   // rank (1-based) of the element looked for
      }
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        L.hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = L.prefix;
        const unsigned mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = tid; i < n_kept; i += kThreads) {
          const unsigned key = __float_as_uint(sd2[i]);
          if ((key & mask) == prefix) atomicAdd(&L.hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned hv = L.hist[tid];
        unsigned incl = wave::scan_incl_dpp(hv);
        if (tid == 0) {
          L.sel_bin = 255u;
          L.sel_acc = 0xFFFFFFFFu;
        }
        wave::block4_publish(L.cnt, lane == 63, incl);
        incl = wave::block4_offset(L.cnt, wv, incl);
        const unsigned excl = incl - hv, kleft = L.kleft;
        if (excl < kleft && kleft <= incl) {   // exactly one bin: 1 <= kleft <= the population
          L.sel_bin = (unsigned)tid;
          L.sel_acc = excl;
        }
        __syncthreads();
        if (tid == 0) {
          unsigned acc = L.sel_acc;
          if (acc == 0xFFFFFFFFu) acc = wave::block4_total(L.cnt);   // rank beyond the population: cannot happen
          L.kleft = L.kleft - acc;
          L.prefix = prefix | (L.sel_bin << shift);
        }
        __syncthreads();
      }
      thr_key = L.prefix;        // the k-th smallest key
      ties_to_take = L.kleft;    // how many elements equal to it belong to the k smallest
    }

    // float64 sums over the selected pairs; ties at the threshold in index order
    double acc[kNSum];
#pragma unroll
    for (int q = 0; q < kNSum; ++q) acc[q] = 0.0;
    unsigned carry = 0;
    for (int b0 = 0; b0 < n_kept; b0 += 4 * kThreads) {
      unsigned key[4];
      bool in[4], sel[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = b0 + 4 * tid + r;
        in[r] = i < n_kept;
        key[r] = in[r] ? __float_as_uint(sd2[i]) : 0xFFFFFFFFu;
      }
      if (thr_key == 0xFFFFFFFFu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sel[r] = in[r];
      } else {
        unsigned mine = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) mine += (in[r] && key[r] == thr_key) ? 1u : 0u;
        const unsigned incl = wave::scan_incl_dpp(mine);
        wave::block4_publish(L.cnt, lane == 63, incl);
        unsigned rank = wave::block4_offset(L.cnt, wv, carry + incl - mine);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool tie = in[r] && key[r] == thr_key;
          sel[r] = in[r] && (key[r] < thr_key || (tie && rank < ties_to_take));
          rank += tie ? 1u : 0u;
        }
        carry += wave::block4_total(L.cnt);
        __syncthreads();   // L.cnt is free again
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = b0 + 4 * tid + r;
        const unsigned jm = in[r] ? (unsigned)sj[i] : 0xFFFFu;
        if (sel[r] && jm != 0xFFFFu) {   // no neighbour below FLT_MAX: never in a sum
          const float px = sx[i], py = sy[i], pz = sz[i];
          const float4 m = ob.model[jm];
          acc[0] += 1.0;
          acc[1] += px; acc[2] += py; acc[3] += pz;
          acc[4] += m.x; acc[5] += m.y; acc[6] += m.z;
          acc[7] += (double)px * m.x; acc[8] += (double)px * m.y; acc[9] += (double)px * m.z;
          acc[10] += (double)py * m.x; acc[11] += (double)py * m.y; acc[12] += (double)py * m.z;
          acc[13] += (double)pz * m.x; acc[14] += (double)pz * m.y; acc[15] += (double)pz * m.z;
          acc[16] += (double)sd2[i];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kNSum; ++q) acc[q] = wave::sum_dpp(acc[q]);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < kNSum; ++q) L.red[wv][q] = acc[q];
    }
    __syncthreads();
    if (tid < kNSum) L.sum[tid] = ((L.red[0][tid] + L.red[1][tid]) + L.red[2][tid]) + L.red[3][tid];   // block4_total's order
    __syncthreads();
    if (tid == 0) {
      const double* red = L.sum;
      const double E = red[0] >= 1.0 ? red[16] / red[0] : 0.0;
      solve_rigid(red, L.G);   // the update first, then the progress tests (PCL's order)
      const double E_old = L.e_old;
      L.e_old = E;
      bool go = it + 1 < a.max_iter;
      if (a.ratio > 0.f && !(E / E_old < (double)a.ratio)) go = false;   // TrimmedICP's energy ratio
      if (red[0] < 1.0) go = false;                                        // no correspondences left
      L.go = go ? 1 : 0;
    }
    __syncthreads();
    ++it;
    e_last = (float)L.e_old;
    if (!L.go) break;
  }

  // ---- 5. write back ----
  if (tid == 0) {
    float To[16];
    rigid_inverse(L.G, To);
#pragma unroll
    for (int q = 0; q < 16; ++q) Tg[q] = To[q];
    if (a.energy) a.energy[state] = e_last;
    if (a.iters) a.iters[state] = it;
    if (a.n_kept) a.n_kept[state] = n_kept;
  }
}

}  // namespace

int check_tricp_options(const pgp_tricp_options* o, const char* who, pgp_tricp_options& out) {
  if (!o) {
    pgp_tricp_default_options(&out);
    return PGP_OK;
  }
  if (!std::isfinite(o->trim_fraction) || !(o->trim_fraction > 0.f) || o->trim_fraction > 1.f) {
    set_error("%s: trim_fraction %g outside (0, 1]", who, (double)o->trim_fraction);
    return PGP_EINVAL;
  }
  if (!std::isfinite(o->removal_radius) || !std::isfinite(o->energy_ratio)) {
    set_error("%s: removal_radius and energy_ratio must be finite", who);
    return PGP_EINVAL;
  }
  if (o->max_iterations > 1000) {
    set_error("%s: max_iterations %d above 1000", who, o->max_iterations);
    return PGP_EINVAL;
  }
  out = *o;
  if (out.max_iterations <= 0) out.max_iterations = 100;
  return PGP_OK;
}

int launch_tricp_states(pgp_ctx* ctx, const pgp_tricp_options& o, int n_states, const int* d_obj, int obj_uniform, float* d_T,
                        const int* d_soff, const int* d_sobj, const float* d_sT, float* d_energy, int* d_iters,
                        int* d_n_kept, hipStream_t st) {
  if (n_states <= 0) return PGP_OK;
  if (ctx->tricp_n_obj <= 0) {
    set_error("trimmed ICP of states: no object set (pgp_tricp_set_objects)");
    return PGP_ESTATE;
  }
  TricpArgs a{};
  a.objs = ctx->d_tricp_objs.as<TricpObject>();
  a.n_obj = ctx->tricp_n_obj;
  a.n_states = n_states;
  a.obj = d_obj;
  a.obj_uniform = obj_uniform;
  a.T = d_T;
  a.soff = d_soff;
  a.sobj = d_sobj;
  a.sT = d_sT;
  a.trim = o.trim_fraction;
  a.r2 = o.removal_radius * o.removal_radius;
  a.ratio = o.energy_ratio;
  a.filter = o.removal_radius > 0.f ? 1 : 0;
  a.max_iter = o.max_iterations;
  a.energy = d_energy;
  a.iters = d_iters;
  a.n_kept = d_n_kept;
  a.cap = std::max(kThreads, (ctx->tricp_max_seg + kThreads - 1) / kThreads * kThreads);
  const size_t lds = sizeof(TricpLds) + (size_t)a.cap * 18;
  if (!ctx->tricp_attr_set) {
    PGP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tricp_states), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(sizeof(TricpLds) + (size_t)PGP_TRICP_MAX_SEGMENT * 18)));
    ctx->tricp_attr_set = true;
  }
  hipLaunchKernelGGL(tricp_states, dim3(n_states), dim3(kThreads), lds, st, a);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

}  // namespace pgp
