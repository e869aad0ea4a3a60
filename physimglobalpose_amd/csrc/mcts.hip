// csrc/mcts.hip -- MCTS hypothesis selection: UCTSearch::performSearch with every state evaluated on the device.
//
// Replaces the node's MCTS verification mode (PPE/data_layer/SceneCfg.cpp:410-421 ->
// hypothesis_verification/HypothesisSelection.cpp:241-265 -> mcts/UCTSearch.cpp, mcts/UCTState.cpp).  The tree and
// the stop rules stay on the host; each step's states are settled (physics.hip), rendered (render.hip) and costed
// (depth_cost.hip) on one stream, one launch per level and stage, with ONE synchronisation per step.  The rules,
// restated operation for operation by tests/_mcts_restate.py:
//
// Tree.  The root has depth 0.  A node at depth d < n_obj has one child per hypothesis of object d (objOrder); the
//   children's hval are that object's LCP scores.  A child's state is its parent's objects plus object d at its
//   settled pose (correctPhysics moves only the newest object, every earlier one is static).
// Selection (treePolicy) runs from the root while depth < n_obj:
//   - a node with an unexpanded child expands one (UCTSearch::expand): hypotheses are scanned in index order and the
//     unexpanded one with hval >= best is kept, from best = 0: the LAST maximum wins.  The new child is settled and
//     rendered; its cost is computed only when it is a leaf (an internal node's renderScore is never read).
//   - otherwise it descends to getBestChild (UCTState.cpp:275-299): children in EXPANSION order,
//       tmp = (float)((double)(q / (float)n) - (double)alpha * sqrt(2 * log((double)N) / (double)n))
//     (N the parent's visit count; q / n a float divide, the rest double, exactly the reference's types), the child
//     kept when tmp < best from best = (float)INT_MAX: strict, the FIRST minimum wins.  Host log / sqrt decide.
//   The selected node is the expanded child, or a leaf reached by descending.
// Rollout (defaultPolicy, UCTSearch.cpp:140-198) from a selected node that is not a leaf adds each remaining object l
//   in order, settled against the state's earlier objects, then rendered:
//     random:  h = sample_variate(sample_state(seed, t), l) % n_hyp[l]   (pgp_internal.h; t = the descent's global
//              0-based index.  The reference's process-global rand() is replaced on purpose.)
//     LCP:     (LCPPolicy, :73-135) the first index with score > best from best = 0; all scores zero -> index 0.
//   The leaf's cost is computeCost (UCTState.cpp:93-116) of the merged image.
// A leaf selected again is not evaluated: its reward is its stored score.
// Backup (backupReward) from the selected node to the root: n += 1, q = q + reward (float); reward = (float)renderScore.
// Best state: strict <, from +inf, the earlier candidate kept on ties; candidates in descent order (per descent its
//   expanded child when that is a leaf, else its rollout leaf).
// Batching (leaves_per_step B > 1): a step makes up to B descents one after the other on the host tree.  Each adds an
//   in-flight visit v += 1 to every node of its path before the next descent selects; selection uses n' = n + v,
//   q' = q + (float)v * V, N' = N + v_parent.  A node expanded earlier in the step counts as expanded (later descents
//   take the next child, or descend through it once its parent is full).  A leaf expanded earlier in the step and
//   selected again gets its reward once the step has evaluated it.  After the step's evaluation the backups run in
//   descent order and every v returns to 0.  With B = 1, v is 0 at every selection: the reference's order.
// Stop, checked before each descent: expansions >= max_expansions (the reference's test); descents == max_iterations;
//   every node expanded (the tree is exhausted: the reference would only re-back-up leaves).  elapsed > max_seconds is
//   checked after each step.
//
// Device side of a step, for levels l = 0 .. n_obj-1 (each slot = one evaluated descent, one full leaf state):
//   mcts_gather   builds the settle inputs of the states that ADD object l this step (expanded children of depth
//                 l + 1 and rollout levels): the hypothesis pose from HBM, the statics = the slot's poses of levels < l.
//   tricp_states  only with pgp_mcts_set_tricp on: one launch refines the gathered poses in place against the slot's
//                 placed objects (tricp_states.hip: performTrICP, UCTSearch.cpp:98, 157, 225); off: not launched.
//   settle_kernel one launch for all of them (physics.hip).
//   mcts_scatter  writes each slot's pose of level l (settled now, or an ancestor's from the node-pose arena) into the
//                 slot's pose table and the render batch, and new nodes' settled poses into the arena.
//   render        object l for EVERY slot under the slot's image of level l - 1 (two images per slot, alternating:
//                 render_init reads the parent).  Re-rendering the ancestors gives copyParent's image bit for bit: the
//                 z-buffer is an atomic min of positive depths and the parent merge (UCTState.cpp:62-68) is the same
//                 min, so the order of the objects does not matter.  A node stores 16 floats, not an image.
// then one depth_cost launch over the slots' leaf images; only the scores come home, and the best leaf's poses at the
// end (a device-to-device copy of its slot's pose table whenever the best improves).

#include "pgp_internal.h"

#include <chrono>
#include <climits>
#include <cmath>

namespace pgp {

namespace {

// settle inputs of level l: one workgroup per state k = list[3k] slot, list[3k+1] global hypothesis row
__global__ __launch_bounds__(64) void mcts_gather(int l, int n_obj, const int* __restrict__ shape, const int* __restrict__ list,
                                                  int n_settle, const float* __restrict__ hypT,
                                                  const float* __restrict__ slot_pose, int* __restrict__ dyn,
                                                  float* __restrict__ T, int* __restrict__ off, int* __restrict__ ss,
                                                  float* __restrict__ sT) {
  const int k = blockIdx.x;
  if (k >= n_settle) return;
  const int s = list[3 * k], row = list[3 * k + 1];
  const int tid = threadIdx.x;
  if (tid < 16) T[16 * (size_t)k + tid] = hypT[16 * (size_t)row + tid];
  if (tid < l) ss[(size_t)k * l + tid] = shape[tid];
  for (int i = tid; i < 16 * l; i += blockDim.x)
    sT[(size_t)k * l * 16 + i] = slot_pose[((size_t)s * n_obj) * 16 + i];   // levels 0 .. l-1 of the slot
  if (tid == 0) {
    dyn[k] = shape[l];
    off[k + 1] = (k + 1) * l;
    if (k == 0) off[0] = 0;
  }
}

// level l's pose of every slot (src >= 0: settle output src; < 0: arena node -src-1) and the arena's new nodes
__global__ __launch_bounds__(256) void mcts_scatter(int l, int n_obj, int n_slots, const int* __restrict__ src,
                                                    const int* __restrict__ list, int n_settle,
                                                    const float* __restrict__ settled, float* __restrict__ arena,
                                                    long long arena_nodes, float* __restrict__ slot_pose,
                                                    float* __restrict__ render_T) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c = (int)(i & 15);
  const long long e = i >> 4;
  if (e < n_slots) {
    const int s = (int)e, from = src[s];
    float v;
    if (from >= 0) {
      v = settled[16 * (size_t)from + c];
    } else {
      const long long node = -(long long)from - 1;
      v = node < arena_nodes ? arena[16 * node + c] : __int_as_float(0x7FC00000);
    }
    slot_pose[((size_t)s * n_obj + l) * 16 + c] = v;
    render_T[16 * (size_t)s + c] = v;
  } else if (e < (long long)n_slots + n_settle) {
    const int k = (int)(e - n_slots);
    const int node = list[3 * k + 2];
    if (node >= 0 && node < arena_nodes) arena[16 * (size_t)node + c] = settled[16 * (size_t)k + c];
  }
}

struct MNode {
  int parent, depth, hyp;               // hyp: the hypothesis of object depth - 1 (-1: the root)
  int n = 0, v = 0;                     // backed-up and in-flight visits
  float q = 0.f;
  float score = 0.f;                    // renderScore (leaves, once evaluated)
  bool evaluated = false;
  int open = 0;                         // unexpanded children left
  int step_idx = -1;                    // expanded in the current step: its index in level depth-1's settle batch
  std::vector<int> children;            // expansion order
  std::vector<unsigned char> expanded;  // per hypothesis of object `depth`
};

struct Descent {
  int t, sel, slot, depth;   // slot -1: a leaf selected again
  int hyp[PGP_MCTS_MAX_OBJECTS];
  std::vector<int> path;     // root .. sel
};

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

bool finite_all(const float* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// device allocations of one search that do not outlive it
struct CallBufs {
  DevBuf arena, hyp, mesh;
  void* pinned = nullptr;
  ~CallBufs() {
    arena.release();
    hyp.release();
    mesh.release();
    if (pinned) (void)hipHostFree(pinned);
  }
};

}  // namespace

int mcts_search_impl(pgp_ctx* ctx, const pgp_mcts_options* opt, const pgp_mcts_object* objs, int n_obj,
                     const float* table_params, const float* cam_pose, const pgp_camera* cam, const float* observed,
                     int* best_hyp, float* best_T, float* best_score, pgp_mcts_info* info, pgp_mcts_record* trace,
                     int trace_cap, int* n_trace) {
  const char* who = "pgp_mcts_search";
  const auto t_begin = std::chrono::steady_clock::now();
  // ---- validation (before any device work) ----
  if (n_obj < 1 || n_obj > PGP_MCTS_MAX_OBJECTS) {
    set_error("%s: n_obj %d outside 1 .. %d", who, n_obj, PGP_MCTS_MAX_OBJECTS);
    return PGP_EINVAL;
  }
  if (!objs || !cam || !observed || !best_hyp || !best_T || !best_score || trace_cap < 0 || (trace_cap > 0 && !trace)) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  if (opt->leaves_per_step < 1 || opt->leaves_per_step > PGP_MCTS_MAX_LEAVES_PER_STEP || !std::isfinite(opt->alpha) ||
      opt->max_iterations <= 0 || !std::isfinite(opt->explanation_threshold) || !(opt->max_seconds >= 0.f) ||
      !std::isfinite(opt->virtual_cost) || (opt->rollout != PGP_MCTS_ROLLOUT_RANDOM && opt->rollout != PGP_MCTS_ROLLOUT_LCP)) {
    set_error("%s: bad options (leaves_per_step 1 .. 256, finite alpha, max_iterations > 0, rollout mode)", who);
    return PGP_EINVAL;
  }
  if (cam->rows <= 0 || cam->cols <= 0 || (size_t)cam->rows * cam->cols > (size_t)1 << 24) {
    set_error("%s: bad image size %d x %d", who, cam->rows, cam->cols);
    return PGP_EINVAL;
  }
  int rc = check_options(&opt->physics, who, PHYS_MAX_STEPS);
  if (rc != PGP_OK) return rc;
  PhysParams P;
  if ((rc = make_params(ctx, &opt->physics, 0, table_params, cam_pose, who, P)) != PGP_OK) return rc;
  const int n_shapes = (int)ctx->phys_shapes.size();
  std::vector<int> n_hyp(n_obj), hyp_off(n_obj + 1, 0), shape(n_obj);
  for (int l = 0; l < n_obj; ++l) {
    const pgp_mcts_object& o = objs[l];
    if (o.shape_id < 0 || o.shape_id >= n_shapes) {
      set_error("%s: object %d names shape %d of %d", who, l, o.shape_id, n_shapes);
      return PGP_EINVAL;
    }
    if (o.n_hyp < 1 || !o.T || !o.scores || !finite_all(o.T, (size_t)o.n_hyp * 16)) {
      set_error("%s: object %d needs n_hyp >= 1 finite poses and scores", who, l);
      return PGP_EINVAL;
    }
    for (int h = 0; h < o.n_hyp; ++h)
      if (!std::isfinite(o.scores[h]) || o.scores[h] < 0.f) {   // NaN, +-inf or negative
        set_error("%s: object %d hypothesis %d has score %g (finite, >= 0 expected)", who, l, h, (double)o.scores[h]);
        return PGP_EINVAL;
      }
    if ((o.vertex_stride != 3 && o.vertex_stride != 4) || o.n_vert < 0 || o.n_tri < 0 || (o.n_vert > 0 && !o.vertices) ||
        !finite_all(o.vertices, (size_t)o.n_vert * o.vertex_stride)) {
      set_error("%s: object %d has a bad mesh", who, l);
      return PGP_EINVAL;
    }
    if (o.triangles)
      for (size_t i = 0; i < (size_t)o.n_tri * 3; ++i)
        if (o.triangles[i] < 0 || o.triangles[i] >= o.n_vert) {
          set_error("%s: object %d triangle index %d outside 0 .. %d", who, l, o.triangles[i], o.n_vert - 1);
          return PGP_EINVAL;
        }
    n_hyp[l] = o.n_hyp;
    hyp_off[l + 1] = hyp_off[l] + o.n_hyp;
    shape[l] = o.shape_id;
  }
  // pgp_mcts_set_tricp: object l of the search is object l of the resident set
  const bool tricp = ctx->mcts_tricp;
  if (tricp && ctx->tricp_n_obj != n_obj) {
    set_error("%s: trimmed ICP is switched on and the context holds %d objects (pgp_tricp_set_objects), the search %d", who,
              ctx->tricp_n_obj, n_obj);
    return PGP_EINVAL;
  }
  // stop limits: the reference's sum_{i=0..n_obj} 25^i, clamped; the tree's node count (saturating)
  long long max_exp = opt->max_expansions;
  if (max_exp <= 0) {
    double s = 0.0;
    for (int i = 0; i <= n_obj; ++i) s += std::pow(25.0, i);
    max_exp = s >= 2147483647.0 ? 2147483647LL : (long long)s;
  }
  long long total_nodes = 0;
  {
    long double width = 1.0L, sum = 0.0L;
    for (int l = 0; l < n_obj; ++l) {
      width *= n_hyp[l];
      sum += width;
    }
    total_nodes = sum >= 9.0e18L ? LLONG_MAX : (long long)sum;
  }
  const int B = opt->leaves_per_step;
  const float V = opt->virtual_cost > 0.f ? opt->virtual_cost : (float)((double)cam->rows * cam->cols);
  const size_t n_pix = (size_t)cam->rows * cam->cols;
  hipStream_t st = ctx->stream;

  // ---- device buffers: persistent workspace + images, per-call hypotheses, meshes, arena ----
  CallBufs cb;
  const size_t b_hyp = al256((size_t)hyp_off[n_obj] * 64);
  std::vector<size_t> v_off(n_obj), t_off(n_obj);
  size_t b_mesh = 0;
  for (int l = 0; l < n_obj; ++l) {
    v_off[l] = b_mesh;
    b_mesh += al256((size_t)std::max(objs[l].n_vert, 1) * objs[l].vertex_stride * 4);
    t_off[l] = b_mesh;
    b_mesh += al256((size_t)std::max(objs[l].triangles ? objs[l].n_tri : 0, 1) * 12);
  }
  if ((rc = cb.hyp.ensure(b_hyp + al256((size_t)n_obj * 4))) != PGP_OK) return rc;
  if ((rc = cb.mesh.ensure(b_mesh)) != PGP_OK) return rc;
  const size_t nl = (size_t)n_obj;
  const size_t b_slot_pose = al256((size_t)B * nl * 64), b_rT = al256((size_t)B * 64), b_dyn = al256((size_t)B * 4),
               b_T = al256((size_t)B * 64), b_off = al256((size_t)(B + 1) * 4), b_ss = al256((size_t)B * 16 * 4),
               b_sT = al256((size_t)B * 16 * 64), b_out = al256((size_t)B * 64), b_cnt = al256((size_t)B * 12),
               b_sc = al256((size_t)B * 4), b_best = al256(nl * 64), b_obs = al256(n_pix * 4),
               b_desc = al256((size_t)nl * B * 4 * 4);
  const size_t ws_total = b_slot_pose + b_rT + b_dyn + b_T + b_off + b_ss + b_sT + b_out + b_cnt + b_sc + b_best + b_obs + b_desc;
  if ((rc = ctx->d_mcts_ws.ensure(ws_total)) != PGP_OK) return rc;
  if ((rc = ctx->d_mcts_img.ensure(2 * (size_t)B * n_pix * 4)) != PGP_OK) return rc;
  unsigned char* w = ctx->d_mcts_ws.as<unsigned char>();
  float* d_slot_pose = reinterpret_cast<float*>(w);
  w += b_slot_pose;
  float* d_render_T = reinterpret_cast<float*>(w);
  w += b_rT;
  int* d_dyn = reinterpret_cast<int*>(w);
  w += b_dyn;
  float* d_T = reinterpret_cast<float*>(w);
  w += b_T;
  int* d_off = reinterpret_cast<int*>(w);
  w += b_off;
  int* d_ss = reinterpret_cast<int*>(w);
  w += b_ss;
  float* d_sT = reinterpret_cast<float*>(w);
  w += b_sT;
  float* d_out = reinterpret_cast<float*>(w);
  w += b_out;
  int* d_counts = reinterpret_cast<int*>(w);
  w += b_cnt;
  float* d_scores = reinterpret_cast<float*>(w);
  w += b_sc;
  float* d_best = reinterpret_cast<float*>(w);
  w += b_best;
  float* d_obs = reinterpret_cast<float*>(w);
  w += b_obs;
  int* d_desc = reinterpret_cast<int*>(w);
  float* d_img[2] = {ctx->d_mcts_img.as<float>(), ctx->d_mcts_img.as<float>() + (size_t)B * n_pix};
  float* d_hypT = cb.hyp.as<float>();
  int* d_shape = reinterpret_cast<int*>(cb.hyp.as<unsigned char>() + b_hyp);
  // pinned host staging: the step's descriptors (levels x (3 B settle + B src) ints) and scores
  const size_t h_desc_ints = nl * (size_t)B * 4;
  PGP_HIP(hipHostMalloc(&cb.pinned, h_desc_ints * 4 + (size_t)B * 4, hipHostMallocDefault));
  int* h_desc = static_cast<int*>(cb.pinned);
  float* h_scores = reinterpret_cast<float*>(h_desc + h_desc_ints);

  for (int l = 0; l < n_obj; ++l) {
    PGP_HIP(hipMemcpyAsync(d_hypT + (size_t)hyp_off[l] * 16, objs[l].T, (size_t)n_hyp[l] * 64, hipMemcpyHostToDevice, st));
    if (objs[l].n_vert > 0)
      PGP_HIP(hipMemcpyAsync(cb.mesh.as<unsigned char>() + v_off[l], objs[l].vertices,
                             (size_t)objs[l].n_vert * objs[l].vertex_stride * 4, hipMemcpyHostToDevice, st));
    if (objs[l].triangles && objs[l].n_tri > 0)
      PGP_HIP(hipMemcpyAsync(cb.mesh.as<unsigned char>() + t_off[l], objs[l].triangles, (size_t)objs[l].n_tri * 12,
                             hipMemcpyHostToDevice, st));
  }
  PGP_HIP(hipMemcpyAsync(d_shape, shape.data(), nl * 4, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_obs, observed, n_pix * 4, hipMemcpyHostToDevice, st));
  // node-pose arena: grows by doubling, its contents kept
  long long arena_cap = std::min<long long>(std::max<long long>(std::min(total_nodes, (long long)opt->max_iterations), 1) + 1, 4096);
  if ((rc = cb.arena.ensure((size_t)arena_cap * 64)) != PGP_OK) return rc;

  // ---- host tree ----
  std::vector<MNode> nodes;
  nodes.reserve((size_t)std::min<long long>(arena_cap, 1 << 20));
  auto new_node = [&](int parent, int depth, int hyp) {
    MNode m;
    m.parent = parent;
    m.depth = depth;
    m.hyp = hyp;
    if (depth < n_obj) {
      m.open = n_hyp[depth];
      m.expanded.assign((size_t)n_hyp[depth], 0);
    }
    nodes.push_back(std::move(m));
    return (int)nodes.size() - 1;
  };
  new_node(-1, 0, -1);
  int lcp_pick[PGP_MCTS_MAX_OBJECTS];
  for (int l = 0; l < n_obj; ++l) {
    int bi = 0;
    float bs = 0.f;
    for (int h = 0; h < n_hyp[l]; ++h)
      if (objs[l].scores[h] > bs) {
        bs = objs[l].scores[h];
        bi = h;
      }
    lcp_pick[l] = bi;
  }

  long long descents = 0, expansions = 0, steps = 0, settles = 0;
  int stop = 0;
  float best = INFINITY;
  int best_slot_hyp[PGP_MCTS_MAX_OBJECTS];
  for (int l = 0; l < PGP_MCTS_MAX_OBJECTS; ++l) best_slot_hyp[l] = -1;
  std::vector<Descent> ds;
  std::vector<int> slot_desc, slot_d0, own_k;   // per slot: its descent, its first new level, its settle index
  std::vector<int> level_base(n_obj), level_n(n_obj), src_base(n_obj);
  while (!stop) {
    // ---- the step's descents on the host tree ----
    ds.clear();
    slot_desc.clear();
    slot_d0.clear();
    if ((long long)nodes.size() + B > arena_cap) {   // grow the arena before this step's launches
      long long cap = arena_cap;
      while ((long long)nodes.size() + B > cap) cap *= 2;
      DevBuf nb;
      if ((rc = nb.ensure((size_t)cap * 64)) != PGP_OK) return rc;
      PGP_HIP(hipMemcpyAsync(nb.p, cb.arena.p, (size_t)nodes.size() * 64, hipMemcpyDeviceToDevice, st));
      PGP_HIP(hipStreamSynchronize(st));
      cb.arena.release();
      cb.arena = nb;
      arena_cap = cap;
    }
    for (int b = 0; b < B; ++b) {
      if (expansions >= max_exp) { stop = PGP_MCTS_STOP_EXPANSIONS; break; }
      if (descents == (long long)opt->max_iterations) { stop = PGP_MCTS_STOP_ITERATIONS; break; }
      if (expansions >= total_nodes) { stop = PGP_MCTS_STOP_EXHAUSTED; break; }
      Descent D;
      D.t = (int)descents++;
      D.slot = -1;
      for (int l = 0; l < PGP_MCTS_MAX_OBJECTS; ++l) D.hyp[l] = -1;
      int cur = 0;
      D.path.push_back(0);
      int sel = -1;
      bool expanded_now = false;
      while (nodes[cur].depth < n_obj) {
        if (nodes[cur].open > 0) {   // expand: the last unexpanded maximum of hval
          const int d = nodes[cur].depth;
          int bi = -1;
          float bh = 0.f;
          for (int h = 0; h < n_hyp[d]; ++h)
            if (!nodes[cur].expanded[h] && objs[d].scores[h] >= bh) {
              bh = objs[d].scores[h];
              bi = h;
            }
          const int c = new_node(cur, d + 1, bi);
          nodes[cur].expanded[bi] = 1;
          nodes[cur].open -= 1;
          nodes[cur].children.push_back(c);
          ++expansions;
          D.path.push_back(c);
          sel = c;
          expanded_now = true;
          break;
        }
        // getBestChild over expansion order, first minimum; virtual visits folded in
        const MNode& p = nodes[cur];
        const double logN = std::log((double)(p.n + p.v));
        int bc = -1;
        float bv = (float)INT_MAX;
        for (int c : p.children) {
          const MNode& ch = nodes[c];
          const int np = ch.n + ch.v;
          const float qp = ch.q + (float)ch.v * V;
          const float tmp = (float)((double)(qp / (float)np) - (double)opt->alpha * std::sqrt(2.0 * logN / (double)np));
          if (tmp < bv) {
            bv = tmp;
            bc = c;
          }
        }
        if (bc < 0) bc = p.children[0];   // every value NaN: cannot happen with finite alpha and n' >= 1
        cur = bc;
        D.path.push_back(cur);
      }
      if (sel < 0) sel = cur;   // a leaf selected again
      D.sel = sel;
      D.depth = nodes[sel].depth;
      for (size_t i = 1; i < D.path.size(); ++i) D.hyp[nodes[D.path[i]].depth - 1] = nodes[D.path[i]].hyp;
      for (int x : D.path) nodes[x].v += 1;
      if (expanded_now) {   // evaluated this step: the new child's level and the rollout levels
        for (int l = D.depth; l < n_obj; ++l)
          D.hyp[l] = opt->rollout == PGP_MCTS_ROLLOUT_LCP ? lcp_pick[l]
                                                          : (int)(sample_variate(sample_state(opt->seed, D.t), l) % (unsigned)n_hyp[l]);
        D.slot = (int)slot_desc.size();
        slot_desc.push_back((int)ds.size());
        slot_d0.push_back(D.depth - 1);
      }
      ds.push_back(std::move(D));
    }
    if (ds.empty()) break;
    const int n_slots = (int)slot_desc.size();

    // ---- the step's device work ----
    if (n_slots > 0) {
      // descriptors: per level, 3 ints per settle state (slot, hypothesis row, arena node or -1), then 1 src per slot
      int* h = h_desc;
      own_k.assign((size_t)n_slots, -1);
      for (int l = 0; l < n_obj; ++l) {
        level_base[l] = (int)(h - h_desc);
        int k = 0;
        for (int s = 0; s < n_slots; ++s) {
          const Descent& D = ds[slot_desc[s]];
          if (slot_d0[s] > l) continue;
          h[3 * k] = s;
          h[3 * k + 1] = hyp_off[l] + D.hyp[l];
          h[3 * k + 2] = slot_d0[s] == l ? D.sel : -1;
          if (slot_d0[s] == l) nodes[D.sel].step_idx = k;
          own_k[s] = k;
          ++k;
        }
        level_n[l] = k;
        h += 3 * k;
        src_base[l] = (int)(h - h_desc);
        for (int s = 0; s < n_slots; ++s) {
          const Descent& D = ds[slot_desc[s]];
          int v;
          if (slot_d0[s] <= l) {
            v = own_k[s];
          } else {
            const int a = D.path[l + 1];   // the ancestor that adds object l
            v = nodes[a].step_idx >= 0 ? nodes[a].step_idx : -(a + 1);
          }
          h[s] = v;
        }
        h += n_slots;
      }
      const size_t n_desc = (size_t)(h - h_desc);
      PGP_HIP(hipMemcpyAsync(d_desc, h_desc, n_desc * 4, hipMemcpyHostToDevice, st));
      for (int l = 0; l < n_obj; ++l) {
        const int ns = level_n[l];
        const int* d_list = d_desc + level_base[l];
        if (ns > 0) {
          hipLaunchKernelGGL(mcts_gather, dim3(ns), dim3(64), 0, st, l, n_obj, (const int*)d_shape, d_list, ns,
                             (const float*)d_hypT, (const float*)d_slot_pose, d_dyn, d_T, d_off, d_ss, d_sT);
          PGP_HIP(hipGetLastError());
          // performTrICP (UCTSearch.cpp:98, 157, 225: expand, defaultPolicy, LCPPolicy): every state the level settles is
          // refined first, in place, against its slot's placed objects 0 .. l-1
          if (tricp && (rc = launch_tricp_states(ctx, ctx->mcts_tricp_opt, ns, nullptr, l, d_T, d_off, nullptr, d_sT, nullptr,
                                                 nullptr, nullptr, st)) != PGP_OK)
            return rc;
          P.n_states = ns;
          if ((rc = launch_settle(ctx, P, d_dyn, d_T, d_off, d_ss, d_sT, d_out, nullptr, nullptr, nullptr, nullptr, st)) != PGP_OK)
            return rc;
          settles += ns;
        }
        const long long threads = 16LL * (n_slots + ns);
        hipLaunchKernelGGL(mcts_scatter, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, l, n_obj, n_slots,
                           (const int*)(d_desc + src_base[l]), d_list, ns, (const float*)d_out, cb.arena.as<float>(),
                           arena_cap, d_slot_pose, d_render_T);
        PGP_HIP(hipGetLastError());
        const pgp_mcts_object& o = objs[l];
        const float* verts = reinterpret_cast<const float*>(cb.mesh.as<unsigned char>() + v_off[l]);
        const int* tris = o.triangles ? reinterpret_cast<const int*>(cb.mesh.as<unsigned char>() + t_off[l]) : nullptr;
        if ((rc = launch_render_depth(ctx, verts, o.vertex_stride, o.n_vert, tris, o.n_tri, d_render_T, n_slots, cam,
                                      l > 0 ? d_img[(l - 1) & 1] : nullptr, n_pix, d_img[l & 1], st)) != PGP_OK)
          return rc;
      }
      if ((rc = launch_depth_cost(ctx, d_obs, d_img[(n_obj - 1) & 1], n_slots, (int)n_pix, opt->explanation_threshold,
                                  d_counts, st)) != PGP_OK)
        return rc;
      if ((rc = launch_cost_scores(d_counts, n_slots, d_scores, st)) != PGP_OK) return rc;
      PGP_HIP(hipMemcpyAsync(h_scores, d_scores, (size_t)n_slots * 4, hipMemcpyDeviceToHost, st));
      PGP_HIP(hipStreamSynchronize(st));
    }
    // ---- results, best state, backups (descent order) ----
    int best_slot = -1;
    for (Descent& D : ds) {
      if (D.slot < 0) continue;
      const float sc = h_scores[D.slot];
      if (D.depth == n_obj) {
        nodes[D.sel].score = sc;
        nodes[D.sel].evaluated = true;
      }
      if (sc < best) {
        best = sc;
        best_slot = D.slot;
        for (int l = 0; l < PGP_MCTS_MAX_OBJECTS; ++l) best_slot_hyp[l] = D.hyp[l];
      }
    }
    if (best_slot >= 0)
      PGP_HIP(hipMemcpyAsync(d_best, d_slot_pose + (size_t)best_slot * nl * 16, nl * 64, hipMemcpyDeviceToDevice, st));
    for (const Descent& D : ds) {
      const float reward = D.slot >= 0 ? h_scores[D.slot] : nodes[D.sel].score;
      for (int x : D.path) {
        nodes[x].n += 1;
        nodes[x].q = nodes[x].q + reward;
        nodes[x].v = 0;
      }
      if (trace && D.t < trace_cap) {
        pgp_mcts_record& r = trace[D.t];
        r.step = (int)steps;
        r.t = D.t;
        r.depth = D.depth;
        for (int l = 0; l < PGP_MCTS_MAX_OBJECTS; ++l) r.hyp[l] = D.hyp[l];
        r.evaluated = D.slot >= 0 ? 1 : 0;
        r.render_score = reward;
        r.reward = reward;
      }
    }
    for (const Descent& D : ds) nodes[D.sel].step_idx = -1;
    ++steps;
    if (!stop && opt->max_seconds > 0.f) {
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
      if (el > (double)opt->max_seconds) stop = PGP_MCTS_STOP_TIME;
    }
  }
  // ---- the best leaf ----
  PGP_HIP(hipMemcpyAsync(best_T, d_best, nl * 64, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  for (int l = 0; l < n_obj; ++l) best_hyp[l] = best_slot_hyp[l];
  *best_score = best;
  if (n_trace) *n_trace = (int)std::min<long long>(descents, INT_MAX);
  if (info) {
    info->descents = descents;
    info->steps = steps;
    info->expansions = expansions;
    info->settle_evaluations = settles;
    info->stop_reason = stop;
    info->elapsed_ms = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  }
  return PGP_OK;
}

}  // namespace pgp
