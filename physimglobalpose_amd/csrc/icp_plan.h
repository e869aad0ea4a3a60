// csrc/icp_plan.h -- which form an ICP call takes: pure host code (no HIP; plain g++ compiles it, tools/icp_plan_print.cc
// and tests/test_icp_plan_cpu.py pin it).  icp.hip reads the environment into an IcpEnv at every launch, asks icp_stage1
// what to build, builds it, asks icp_stage2 for the form and calls that form's launcher.  Every form and every knob of the
// ICP host side is listed here.
#pragma once

#include <climits>
#include <cmath>
#include <cstdio>

#include "../../include/pgp.h"

namespace pgp {

// Limits the kernels set (icp.hip asserts that they agree with its own constants).
constexpr int kPlanPoseSrcMax = 4096;   // the per-pose forms keep every correspondence of a pose in one workgroup's LDS
constexpr int kPlanClassBase = 1024;    // the points-per-thread classes 2 / 3 / 4 are in units of this many source points
constexpr int kPlanSumBlock = 4096;     // source points per block of the sums by block (at 1024 threads per workgroup)
constexpr int kPlanSmoothMax = 8;       // history length of the differential checker
constexpr int kPlanMultiMax = 8;        // jobs of one multi-target launch
constexpr int kPlanPosesMax = 32768;    // poses of one launch: the pose index rides on gridDim.z / .y (<= 65535)
constexpr int kPlanSceneNMax = 64;      // poses of the scene-sized one-launch form (the unit sums of more would be gigabytes)

// The environment knobs of the ICP host side, read at every launch (the tests change them between calls).
struct IcpEnv {
  int nn = 0;                   // PGP_ICP_NN, checker path: 0 unset, 1 "scan" (exhaustive search), 2 "index", 3 another value
  // PGP_ICP_SPLIT, checker path: -1 unset, 0 the legacy persistent kernel (fully asynchronous, graph-capturable), 1 host-
  // driven scan.  Measured (tools/icp_time.py, 2500 x 5000, 10 iterations): the host-driven path wins at every batch size
  // tried -- 1 pose 1.2 vs 7.7 ms, 64 poses 3.6 vs 12.8 ms, 256 poses 9.4 vs 12.9 ms -- so it is the default.
  int split = -1;
  int persist = -1;             // PGP_ICP_PERSIST, checker path: -1 unset, 0 = the index with host-driven iterations
  bool scene_persist = true;    // PGP_ICP_SCENE_PERSIST, checker path: 0 = the scene-sized form host-driven
  bool part = true;             // PGP_ICP_PART, checker path: 0 = one workgroup walks the scene for the sums
  bool open_grid = true;        // PGP_ICP_OPEN_GRID, checker path: 0 = the scan alone on targets beyond the index
  bool multi = true;            // PGP_ICP_MULTI, A/B knob: 0 = a multi-target call goes job by job
  int wgs = 0;                  // PGP_ICP_WGS, A/B knob: 0 unset, else 1 / 2 / 4 workgroups per pose
  bool image_global = false;    // PGP_ICP_IMAGE=global, A/B knob: the index image is read from L2 even where it fits LDS
  double cell = 1.0;            // PGP_ICP_CELL, A/B knob: multiplier of the index's cell edge
  double aspect = 1.8;          // PGP_ICP_ASPECT, A/B knob: the plate shape of the index's cells (>= 1)
  bool vic = true;              // PGP_ICP_VIC, A/B knob: 0 = no vicinity graph (searches only)
  int first_walk = 1;           // PGP_ICP_FIRST_WALK, A/B knob
  unsigned solo_ticks = 1100;   // PGP_ICP_SOLO_TICKS, A/B knob: 11 us (tools/icp_time.py sweep)
  double open_cell = 2.0;       // PGP_ICP_OPEN_CELL, A/B knob: the open grid's cell edge in point spacings
  unsigned scene_wgs = UINT_MAX;   // PGP_ICP_SCENE_WGS, A/B knob: upper bound of the scene-sized form's workgroups
  int scene_sleep = 1;          // PGP_ICP_SCENE_SLEEP, A/B knob: the scene-sized form's polling pause
  bool cooperative = false;     // PGP_COOPERATIVE_LAUNCH, A/B knob: 1 = hipLaunchCooperativeKernel for resident launches
  double wait_ms = 3.0;         // PGP_ICP_WAIT_MS, test hook: the clock bound of the kernels whose workgroups wait for each other
  bool force_lost = false;      // PGP_ICP_FORCE_LOST, test hook: the first meeting of every pose counts as lost
  bool debug = false;           // PGP_ICP_DEBUG, test hook: one line per decision on stderr
};

// The floor of the clock bounds of the kernels whose workgroups wait for each other, in ticks of the 100 MHz counter: 3 ms --
// two orders above an iteration (~25 us), three below the 2 s of round 5.
inline unsigned icp_wait_ticks(const IcpEnv& env) {
  const double t = env.wait_ms * 1e5;
  return (unsigned)(t < 100.0 ? 100.0 : (t > 4.0e9 ? 4.0e9 : t));
}

// k_trim = the trimmed count of a cloud of n_src points
inline int icp_trim_count(const pgp_icp_options* prm, int n_src) {
  float tf = prm->trim_fraction;
  if (!(tf > 0.f) || tf > 1.f) tf = 1.f;
  // float numPoints = trim * size; align(..., abs(numPoints), ...) -> int (UCTState.cpp:176,194)
  int k = (int)fabsf(tf * (float)n_src);
  if (k < 1) k = 1;
  if (k > n_src) k = n_src;
  return k;
}
// the pointmatcher history's length: 0 = the differential checker is off
inline int icp_smooth(const pgp_icp_options* prm) {
  return (prm->min_diff_rot > 0.f && prm->min_diff_trans > 0.f)
             ? (prm->smooth_length < 1 ? 1 : (prm->smooth_length > kPlanSmoothMax ? kPlanSmoothMax : prm->smooth_length))
             : 0;
}
inline bool icp_capped(const pgp_icp_options* prm) { return prm->max_corr_dist > 0.f; }
// the TrimmedICP form: trimming and the energy ratio only (no cap, none of the other stop rules)
inline bool icp_trim_only(const pgp_icp_options* prm) {
  return !icp_capped(prm) &&
         !(prm->transformation_epsilon >= 0.f || prm->relative_mse > 0.f || prm->absolute_mse >= 0.f || icp_smooth(prm) > 0);
}
// points-per-thread class of the per-pose kernels
inline int icp_pir_class(int n_src) { return n_src <= 2 * kPlanClassBase ? 2 : (n_src <= 3 * kPlanClassBase ? 3 : 4); }

struct IcpShape {
  int n = 0, n_src = 0, n_tgt = 0;   // poses, source points, target points
  int n_cus = 0;                     // compute units of the device
  bool capturing = false;            // the stream is being captured
  bool has_normals = false;          // target normals were given
  bool scene_form_off = false;       // the caller redoes a job the scene-sized form lost: host-driven this time
  int sum_block = kPlanSumBlock;     // source points per block of the sums by block
};

struct IcpError {
  int rc = PGP_OK;
  char msg[96] = {0};
};

// step 1 of launch_icp (n > 0)
inline IcpError icp_validate(const pgp_icp_options* prm, const IcpShape& s) {
  IcpError e;
  if (s.n_src <= 0 || s.n_tgt <= 0) snprintf(e.msg, sizeof e.msg, "icp: empty source or target cloud");
  else if (prm->error_metric == 1 && !s.has_normals) snprintf(e.msg, sizeof e.msg, "icp: the point-to-plane metric needs target normals");
  else if (prm->error_metric != 0 && prm->error_metric != 1) snprintf(e.msg, sizeof e.msg, "icp: unknown error metric %d", prm->error_metric);
  if (e.msg[0]) e.rc = PGP_EINVAL;
  return e;
}

// ---- stage 1: before the target index exists -----------------------------------------------------------------------------
enum class IcpWant {
  CappedGrid,     // the uniform grid of the capped search; no index
  IndexPerPose,   // the exact index, sized for one workgroup per pose first (n_src <= 4096), then for the host-driven form
  IndexHost,      // the exact index sized for the host-driven form
  NoIndex         // an exhaustive search (with the open grid where that applies): host-driven, or legacy
};
struct IcpStage1 {
  IcpError err;
  IcpWant want = IcpWant::NoIndex;
  bool legacy = false;   // NoIndex only: the single-launch persistent kernel icp_refine<false> (PGP_ICP_SPLIT=0, no history)
};
inline IcpStage1 icp_stage1(const pgp_icp_options* prm, const IcpShape& s, const IcpEnv& env) {
  IcpStage1 r;
  // grid search: only with a correspondence cap; by default when the scan would be >= 2^27 tests per pose
  bool use_grid = false;
  if (icp_capped(prm)) {
    if (prm->nn_search == 2) use_grid = true;
    else if (prm->nn_search == 0) use_grid = (double)s.n_src * (double)s.n_tgt >= 134217728.0;
  } else if (prm->nn_search == 2) {
    snprintf(r.err.msg, sizeof r.err.msg, "icp: the grid search needs max_corr_dist > 0");
    r.err.rc = PGP_EINVAL;
    return r;
  }
  if (use_grid) {
    r.want = IcpWant::CappedGrid;
    return r;
  }
  // exact index of the static target: the default whenever its image fits a workgroup's LDS.  The
  // exhaustive searches stay as the checker paths (nn_search 1, PGP_ICP_NN=scan, or PGP_ICP_SPLIT set).
  bool want = env.split < 0 && (prm->nn_search == 0 || prm->nn_search == 3);
  if (env.nn == 1) want = false;
  if (env.nn == 2 && prm->nn_search != 1) want = true;
  if (want) {
    // one persistent workgroup per pose keeps all n_src correspondences in LDS; the host-driven path 1024
    r.want = (s.n_src <= kPlanPoseSrcMax && env.persist != 0) ? IcpWant::IndexPerPose : IcpWant::IndexHost;
    return r;
  }
  r.legacy = env.split == 0 && icp_smooth(prm) == 0;
  return r;
}

// ---- stage 2: with the fit of the index ----------------------------------------------------------------------------------
struct IcpFit {
  bool per_pose = false;       // the index sized for one workgroup per pose fits
  bool host = false;           // the index sized for the host-driven form fits
  bool image_in_lds = false;   // its image is copied into LDS (else read from L2)
};
enum class IcpForm {
  PerPose,     // one launch, one workgroup per pose
  Clustered,   // the same launch with 2 or 4 workgroups per pose (resident)
  Scene,       // the scene-sized capped form in one launch (resident)
  Host,        // host-driven iterations
  Legacy       // the single-launch persistent kernel of the exhaustive search
};
enum class IcpSearch { Scan, CappedGrid, OpenGrid, IndexLds, IndexL2 };
struct IcpPlan {
  IcpError err;
  IcpForm form = IcpForm::Host;
  IcpForm fallback = IcpForm::Host;     // when a resident grid does not fit the device
  int wgs_per_pose = 1;                 // Clustered: 2 or 4
  bool trim_only = false;               // per-pose forms: the kernels of the TrimmedICP form
  int pir = 4;                          // per-pose forms: points-per-thread class 2 / 3 / 4
  IcpSearch search = IcpSearch::Scan;   // Host and Scene
  bool part_sums = false;               // Host and Scene: the sums by block (else one workgroup walks the scene)
  int n_blk = 1;                        // blocks of the sums by block
};
inline IcpPlan icp_stage2(const pgp_icp_options* prm, const IcpShape& s, const IcpEnv& env, const IcpStage1& s1, const IcpFit& fit) {
  IcpPlan p;
  const bool index_wanted = s1.want == IcpWant::IndexPerPose || s1.want == IcpWant::IndexHost;
  const bool use_index = index_wanted && (fit.per_pose || fit.host), use_grid = s1.want == IcpWant::CappedGrid;
  if (index_wanted && !use_index && prm->nn_search == 3) {
    snprintf(p.err.msg, sizeof p.err.msg, "icp: the target (%d points) does not fit the LDS index", s.n_tgt);
    p.err.rc = PGP_EINVAL;
    return p;
  }
  const int smooth = icp_smooth(prm);
  const bool capped = icp_capped(prm);
  p.n_blk = (s.n_src + s.sum_block - 1) / s.sum_block;
  if (s1.want == IcpWant::IndexPerPose && fit.per_pose) {
    p.form = p.fallback = IcpForm::PerPose;
    p.search = fit.image_in_lds ? IcpSearch::IndexLds : IcpSearch::IndexL2;
    p.trim_only = icp_trim_only(prm);
    p.pir = icp_pir_class(s.n_src);
    // Few poses: 2 or 4 workgroups per pose share the search (64 poses alone would use 64 of the 256 CUs).  Not while the
    // stream is being captured (the chain's event wait is not for a graph) and not with the pointmatcher history.
    int want_wgs = s.n * 4 <= s.n_cus ? 4 : (s.n * 2 <= s.n_cus ? 2 : 1);
    if (env.wgs) want_wgs = env.wgs == 4 ? 4 : (env.wgs == 2 ? 2 : 1);
    if (want_wgs > 1 && smooth == 0 && s.n * want_wgs <= s.n_cus && s.n_src >= 64 * want_wgs && !s.capturing) {
      p.form = IcpForm::Clustered;
      p.wgs_per_pose = want_wgs;
    }
    return p;
  }
  // the grid, the pointmatcher history and the index all live on the host-driven path
  if (!(env.split != 0 || use_grid || smooth > 0 || use_index)) {
    p.form = p.fallback = IcpForm::Legacy;
    return p;
  }
  // Targets beyond the exact index's 65 535 points, no correspondence cap: a uniform grid answers every query that has a
  // neighbour within a safe radius, the exhaustive scan only the others
  const bool open_grid = !use_grid && !use_index && !capped && s.n_tgt > 65535 && prm->nn_search != 1 && env.open_grid;
  p.search = use_grid ? IcpSearch::CappedGrid
                      : (open_grid ? IcpSearch::OpenGrid : (use_index ? (fit.image_in_lds ? IcpSearch::IndexLds : IcpSearch::IndexL2) : IcpSearch::Scan));
  // Scenes beyond one block of 4096 points, nothing to trim (a cap, or every pair kept): the iteration's sums are formed by
  // one workgroup per block and icp_refine only adds them up
  const bool by_block = p.n_blk > 1 && !(!capped && icp_trim_count(prm, s.n_src) < s.n_src) && env.part;
  p.part_sums = by_block;
  // The capped grid search with sums by block -- the shape of the reference's table alignment -- as ONE launch of resident
  // workgroups: up to 64 poses, not with the pointmatcher history, not while the stream is being captured.
  const bool scene = use_grid && by_block && smooth == 0 && s.n_cus > 0 && s.n <= kPlanSceneNMax && !s.scene_form_off && env.scene_persist &&
                     !s.capturing;
  p.form = scene ? IcpForm::Scene : IcpForm::Host;
  p.fallback = IcpForm::Host;
  return p;
}

// ---- several (segment, target) jobs ----------------------------------------------------------------------------------------
struct IcpMultiJob {
  int n, n_src;
  const void* ctx;   // the context that keeps the job's target index
};
struct IcpMultiPlan {
  int rc = PGP_OK;           // of fit()
  bool one_launch = false;   // else job by job
  int total = 0;             // poses of the one launch
  int pir = 2;               // points-per-thread class, from the largest segment
  bool trim_only = false;
};
// fit(j, first, &rc) builds job j's index (sized for one workgroup per pose) and says whether it fits with its image in LDS;
// `first` is the job's first pose in the launch.  It is called job by job, in order, until one does not fit.
template <class Fit>
inline IcpMultiPlan icp_multi_plan(const pgp_icp_options* prm, const IcpEnv& env, const IcpMultiJob* jobs, int n_jobs, Fit&& fit) {
  IcpMultiPlan m;
  bool one = n_jobs >= 2 && n_jobs <= kPlanMultiMax && prm->error_metric == 0 && icp_smooth(prm) == 0 && prm->nn_search != 1 &&
             prm->nn_search != 2 && env.nn == 0 && env.persist < 0 && env.split < 0 && env.multi;
  // a context keeps ONE target index: two jobs with poses on the same context would have the second build overwrite -- or
  // reallocate -- the image the first job's descriptor points to.  Such jobs run one after the other.
  for (int j = 0; j < n_jobs && one; ++j)
    for (int i = 0; i < j && one; ++i)
      if (jobs[i].n > 0 && jobs[j].n > 0 && jobs[i].ctx == jobs[j].ctx) one = false;
  int max_src = 0;
  for (int j = 0; j < n_jobs && one; ++j) {
    if (jobs[j].n == 0) continue;
    if (jobs[j].n_src > kPlanPoseSrcMax) one = false;
    else if (!fit(j, m.total, &m.rc)) one = false;
    if (m.rc != PGP_OK) return m;
    if (!one) break;
    m.total += jobs[j].n;
    max_src = jobs[j].n_src > max_src ? jobs[j].n_src : max_src;
  }
  m.one_launch = one && m.total > 0 && m.total <= kPlanPosesMax;
  m.pir = icp_pir_class(max_src);
  m.trim_only = icp_trim_only(prm);
  return m;
}

}  // namespace pgp
