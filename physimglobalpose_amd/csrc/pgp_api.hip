// csrc/pgp_api.hip -- the C ABI of include/pgp.h: context, uploads, host-pointer entry points.
// No CPU fallback anywhere: every scoring entry point ends in a HIP kernel launch or an error.

#include "pgp_internal.h"
#include "wave.h"
#include "match_plan.h"

#include <chrono>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

namespace pgp {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

int DevBuf::ensure(size_t bytes) {
  if (bytes <= cap && p) return PGP_OK;
  if (bytes == 0) bytes = 16;
  if (p) {
    hipError_t e = hipFree(p);
    (void)e;
    p = nullptr;
    cap = 0;
  }
  // grow geometrically so repeated calls with slowly growing sizes do not reallocate each time
  size_t want = bytes + bytes / 4;
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    p = nullptr;
    set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PGP_ENOMEM : PGP_EHIP;
  }
  cap = want;
  return PGP_OK;
}

void DevBuf::release() {
  if (p) {
    hipError_t e = hipFree(p);
    (void)e;
  }
  p = nullptr;
  cap = 0;
}

int PinBuf::ensure(size_t bytes) {
  if (bytes <= cap) return PGP_OK;
  release();
  const size_t want = bytes + bytes / 4;
  PGP_HIP(hipHostMalloc(&p, want, flags));
  cap = want;
  return PGP_OK;
}

void PinBuf::release() {
  if (p) {
    hipError_t e = hipHostFree(p);
    (void)e;
  }
  p = nullptr;
  cap = 0;
}

namespace {

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) {
      hipError_t e = hipSetDevice(prev);
      (void)e;
    }
  }
};

// Entry-point guard of a context: selects its device and orders this call behind whatever an earlier
// *_device call queued on the CALLER's stream -- those calls return without synchronising while the
// kernels they launched still read the context's arrays (clouds, index, workspaces), and the host-pointer
// entry points rewrite those arrays on the context's own non-blocking stream.  The *_device call only sets
// a flag; the next host-pointer call (synchronous by contract anyway) drains the device first.  Two things
// that were tried and dropped: an event recorded after every *_device call cost the scoring step 3 us (a
// barrier packet between back-to-back steps); recording it lazily here, on the caller's stream, is unsafe --
// the caller may have destroyed that stream, and HIP dereferences the stale handle.
struct CtxGuard : DeviceGuard {
  // join = false for the *_device entry points themselves: they queue on the caller's stream, behind whatever
  // the caller queued there before, and must not synchronise anything while the caller may be capturing a graph
  // (A call that returned on a completion WORD in host memory -- pgp_score_lcp, pgp::publish_and_wait -- leaves a kernel that
  //  has made its last memory access and is merely retiring: nothing to order against.)
  explicit CtxGuard(pgp_ctx* ctx, bool join = true) : DeviceGuard(ctx->device) {
    if (join && ok && ctx->device_work_pending) {
      (void)hipDeviceSynchronize();
      ctx->device_work_pending = false;
    }
  }
};

// after a *_device entry point has queued work on `stream`
inline void note_device_work(pgp_ctx* ctx, hipStream_t stream) {
  if (stream == ctx->stream) return;
  // a stream that is being captured into a graph runs nothing now; whoever replays the graph orders the
  // replays against later calls on the context
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return;
  ctx->device_work_pending = true;
}

// after the host has synchronised a stream that was made to wait for the side-stream index build (await_index):
// the build is through, so its flag is cleared and its counts are taken over here -- a *_device call that follows
// (possibly on a capturing stream, which can neither query nor wait for the build's event) then finds nothing pending
inline int index_settled(pgp_ctx* ctx) { return ctx->index_pending ? finish_index(ctx) : PGP_OK; }

// The N staged fits of ctx->d_rig: pose (double, first for alignment) | T | rms | status.  The four calls that write them
// size the buffer by `bytes` and launch into these pointers (read AFTER d_rig.ensure: it may move the buffer), and
// pgp_congruent_batch_fetch, which reads the resident fits back later, finds them through the same function.
struct RigFits {
  double* pose;
  float* T;
  float* rms;
  int* status;
  size_t bytes;
};
inline RigFits rig_fits(const pgp_ctx* ctx, size_t N) {
  double* pose = ctx->d_rig.as<double>();
  float* T = reinterpret_cast<float*>(pose + 16 * N);
  float* rms = T + 16 * N;
  return RigFits{pose, T, rms, reinterpret_cast<int*>(rms + N), N * (128 + 64 + 4 + 4)};
}
// ... and their way to the caller's arrays (rms, pose: nullable): through the pinned landing area where there is room, one
// wait for all (pgp::HostOut)
inline int fits_home(pgp_ctx* ctx, const RigFits& fit, size_t N, float* T, double* pose, int* status, float* rms, hipStream_t st) {
  HostOut out(ctx, st);
  int rc;
  if ((rc = out.to(status, fit.status, N * 4)) != PGP_OK || (rms && (rc = out.to(rms, fit.rms, N * 4)) != PGP_OK) ||
      (rc = out.to(T, fit.T, N * 64)) != PGP_OK || (pose && (rc = out.to(pose, fit.pose, N * 128)) != PGP_OK))
    return rc;
  return out.sync();
}

inline uint32_t spread10(uint32_t v) {
  v &= 1023u;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

}  // namespace
}  // namespace pgp

using namespace pgp;

extern "C" {

int pgp_version(void) { return 200; }

const char* pgp_last_error(void) { return g_err; }

int pgp_create(pgp_ctx** out, int device_id) {
  if (!out) {
    set_error("pgp_create: out is NULL");
    return PGP_EINVAL;
  }
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_error("no HIP device available (%s); libpgp has no CPU fallback",
              e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return PGP_ENODEV;
  }
  if (device_id < 0) {
    if (hipGetDevice(&device_id) != hipSuccess) device_id = 0;
  }
  if (device_id >= n) {
    set_error("device %d out of range (%d devices)", device_id, n);
    return PGP_EINVAL;
  }
  DeviceGuard guard(device_id);
  if (!guard.ok) {
    set_error("hipSetDevice(%d) failed", device_id);
    return PGP_ENODEV;
  }
  pgp_ctx* ctx = new pgp_ctx();
  ctx->device = device_id;
  {
    int cus = 0, coop = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0 &&
        hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device_id) == hipSuccess && coop)
      ctx->n_cus = cus;   // 0: the kernels whose workgroups wait for each other stay off (icp.hip launch_resident)
  }
  if (const char* v = getenv("PGP_UNROLL")) ctx->unroll = atoi(v);
  if (const char* v = getenv("PGP_HPB")) ctx->hpb_override = atoi(v);
  if (const char* v = getenv("PGP_REFINE")) ctx->refine_best = atoi(v) != 0;
  if (const char* v = getenv("PGP_NN_PRUNE")) {
    const int m = atoi(v);
    if (m >= 0 && m <= 2) ctx->nn_mode = m;
  }
  e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    delete ctx;
    return PGP_ENODEV;
  }
  int rc = ctx->d_best.ensure(32);
  if (rc == PGP_OK && hipMemset(ctx->d_best.p, 0, 32) != hipSuccess) rc = PGP_EHIP;  // key + ticket armed
  if (rc != PGP_OK) {
    (void)hipStreamDestroy(ctx->stream);
    ctx->d_best.release();
    delete ctx;
    return rc;
  }
  *out = ctx;
  return PGP_OK;
}

int pgp_destroy(pgp_ctx* ctx) {
  if (!ctx) return PGP_OK;
  CtxGuard guard(ctx);
  ctx->deferred_build = nullptr;   // (a build that was never queued)
  if (ctx->stream) {
    hipError_t e = hipStreamSynchronize(ctx->stream);
    (void)e;
  }
  nn_destroy(ctx);   // (awaits a pruning pass still on the build stream)
  {
    hipError_t e = hipSuccess;
    if (ctx->build_stream) {
      e = hipStreamSynchronize(ctx->build_stream);
      if (ctx->build_stream_own) e = hipStreamDestroy(ctx->build_stream);   // (else the device's shared one: it stays)
    }
    if (ctx->ev_index) e = hipEventDestroy(ctx->ev_index);
    if (ctx->ev_build0) e = hipEventDestroy(ctx->ev_build0);
    if (ctx->h_build_counts) e = hipHostFree(ctx->h_build_counts);
    (void)e;
    ctx->build_stream = nullptr;
    ctx->ev_index = ctx->ev_build0 = nullptr;
    ctx->h_build_counts = nullptr;
    ctx->index_pending = false;
  }
  DevBuf* bufs[] = {&ctx->d_P, &ctx->d_Pnw, &ctx->d_cell_start, &ctx->d_cell_tmp, &ctx->d_scan_tmp, &ctx->d_build_scan,
                    &ctx->d_bitmap, &ctx->d_blocktab, &ctx->d_kd_nodes, &ctx->d_kd_pts, &ctx->d_occ_start, &ctx->d_cand, &ctx->d_Q, &ctx->d_Qn, &ctx->d_Qpos, &ctx->d_eo_ws, &ctx->d_T, &ctx->d_partial,
                    &ctx->d_scores, &ctx->d_counts, &ctx->d_best, &ctx->d_rec_ws, &ctx->d_hits, &ctx->d_seq, &ctx->d_Qs, &ctx->d_ids,
                    &ctx->d_rig, &ctx->d_icp_src, &ctx->d_icp_tgt, &ctx->d_icp_tgt_n, &ctx->d_icp_grid, &ctx->d_icp_T, &ctx->d_icp_out, &ctx->d_icp_ws, &ctx->d_icp_x, &ctx->d_Qs_unit, &ctx->d_cs_cnt, &ctx->d_cs_entries, &ctx->d_cs_keys,
                    &ctx->d_cs_pairs, &ctx->d_cs_out, &ctx->d_ppf_keys, &ctx->d_ppf_val, &ctx->d_ppf_off, &ctx->d_ppf_pairs, &ctx->d_prob_cdf, &ctx->d_sel_ws, &ctx->d_csb, &ctx->d_csb_picks, &ctx->d_pre_ws, &ctx->d_vg_ws, &ctx->d_mls_ws, &ctx->d_plane_ws, &ctx->d_plane_io, &ctx->d_cc_ws, &ctx->d_cc_io, &ctx->d_crease_ws, &ctx->d_ppf_model, &ctx->d_ppf_alpha, &ctx->d_ppf_ws, &ctx->d_ppf_io, &ctx->d_phys_shapes, &ctx->d_phys_verts, &ctx->d_phys_planes, &ctx->d_phys_io, &ctx->d_mcts_ws, &ctx->d_mcts_img, &ctx->d_pre_io, &ctx->d_depth, &ctx->d_render_ws, &ctx->d_render_io, &ctx->d_cl_keys, &ctx->d_cl_ws, &ctx->d_cl_io, &ctx->d_bp, &ctx->d_top_ws, &ctx->d_pub_ticket,
                    &ctx->d_tricp_clouds, &ctx->d_tricp_objs, &ctx->d_tricp_io,
                    &ctx->d_v4_sel, &ctx->d_v4_mat, &ctx->d_v4_ws, &ctx->d_v4_quads, &ctx->d_v4_picks, &ctx->d_v4_io,
                    &ctx->d_s4_sel, &ctx->d_s4_ws, &ctx->d_s4_pairs, &ctx->d_s4_io, &ctx->d_Prgb, &ctx->d_Qs_nrm, &ctx->d_Qs_rgb,
                    &ctx->d_prep_ws, &ctx->d_fps_ws, &ctx->d_prep_io,
                    &ctx->d_seg_ws, &ctx->d_seg_c, &ctx->d_seg_cloud, &ctx->d_seg_leaves, &ctx->d_seg_rows};
  for (DevBuf* b : bufs) b->release();
  ctx->d_out.release();
  for (PinBuf* b : {&ctx->h_pin, &ctx->h_sel_pin, &ctx->h_w_pin, &ctx->h_s_pin}) b->release();
  if (ctx->h_flag) {
    hipError_t e = hipHostFree(ctx->h_flag);
    (void)e;
    ctx->h_flag = nullptr;
  }
  if (ctx->h_out) {
    hipError_t e = hipHostFree(ctx->h_out);
    (void)e;
    ctx->h_out = nullptr;
  }
  if (ctx->ev_s) {
    hipError_t e = hipEventDestroy(ctx->ev_s);
    (void)e;
    ctx->ev_s = nullptr;
  }
  if (ctx->ev_w) {
    hipError_t e = hipEventDestroy(ctx->ev_w);
    (void)e;
    ctx->ev_w = nullptr;
  }
  for (hipEvent_t e : ctx->ev) {
    hipError_t r = hipEventDestroy(e);
    (void)r;
  }
  if (ctx->stream) {
    hipError_t e = hipStreamDestroy(ctx->stream);
    (void)e;
  }
  delete ctx;
  return PGP_OK;
}

int pgp_center(float* P, int nP, float* Qs, int nQs, float* Qv, int nQv, float centroid_P[3],
               float centroid_Q[3]) {
  if (nP < 0 || nQs < 0 || nQv < 0 || (nP && !P) || (nQs && !Qs) || (nQv && !Qv) || !centroid_P ||
      !centroid_Q) {
    set_error("pgp_center: bad argument");
    return PGP_EINVAL;
  }
  // base.cc:242-249: centroid += pos (index order, float), then /= Scalar(n)
  float cP[3] = {0.f, 0.f, 0.f}, cQ[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < nP; ++i)
    for (int k = 0; k < 3; ++k) cP[k] += P[3 * (size_t)i + k];
  for (int k = 0; k < 3; ++k) cP[k] /= (float)nP;
  for (int i = 0; i < nQs; ++i)
    for (int k = 0; k < 3; ++k) cQ[k] += Qs[3 * (size_t)i + k];
  for (int k = 0; k < 3; ++k) cQ[k] /= (float)nQs;
  // base.cc:256-264
  for (int i = 0; i < nP; ++i)
    for (int k = 0; k < 3; ++k) P[3 * (size_t)i + k] -= cP[k];
  for (int i = 0; i < nQs; ++i)
    for (int k = 0; k < 3; ++k) Qs[3 * (size_t)i + k] -= cQ[k];
  for (int i = 0; i < nQv; ++i)
    for (int k = 0; k < 3; ++k) Qv[3 * (size_t)i + k] -= cQ[k];
  for (int k = 0; k < 3; ++k) {
    centroid_P[k] = cP[k];
    centroid_Q[k] = cQ[k];
  }
  return PGP_OK;
}

namespace {
// the pixel of one scene point as Match4PCSBase::init computes it (base.cc:317-340); false = outside the image
inline bool image_pixel(const float* p, const float cP[3], const float K[9], int rows, int cols, int* row, int* col) {
  // b_ii.pos() += centroid_P_ (float), then double x1,y1,z1 -> Eigen::Vector3f(x1,y1,z1) (back to float)
  const float x = p[0] + cP[0], y = p[1] + cP[1], z = p[2] + cP[2];
  // camIntrinsic * v: Eigen evaluates a 3x3 * 3x1 float product as k0*x + (k1*y + k2*z) per row
  float u[3];
  for (int r = 0; r < 3; ++r) {
    float a = K[3 * r] * x, b = K[3 * r + 1] * y, c = K[3 * r + 2] * z;
    float bc = b + c;
    u[r] = a + bc;
  }
  const float fc = u[0] / u[2], fr = u[1] / u[2];
  // int col = point2D[0]/point2D[2]: truncation toward zero; guard what the reference leaves undefined
  const bool ok = fc == fc && fr == fr && fc > -1.f && fr > -1.f && fc < (float)cols && fr < (float)rows;
  if (!ok) return false;
  *col = (int)fc;
  *row = (int)fr;
  return *col >= 0 && *row >= 0 && *col < cols && *row < rows;
}
}  // namespace

int pgp_weights_from_image(const float* P, int n, const float cP[3], const float K[9],
                           const unsigned short* img, int rows, int cols, float* weights) {
  if (n < 0 || rows < 0 || cols < 0 || (n > 0 && (!P || !weights)) || !cP || !K || (rows * cols > 0 && !img)) {
    set_error("pgp_weights_from_image: bad argument");
    return PGP_EINVAL;
  }
  for (int i = 0; i < n; ++i) {
    int row = 0, col = 0;
    weights[i] = image_pixel(P + 3 * (size_t)i, cP, K, rows, cols, &row, &col) ? (float)img[(size_t)row * cols + col] / 10000 : 0.f;
  }
  return PGP_OK;
}

int pgp_image_rows_needed(const float* P, int n, const float cP[3], const float K[9], int rows, int cols, int* row_min,
                          int* row_max) {
  if (n < 0 || rows < 0 || cols < 0 || (n > 0 && !P) || !cP || !K || !row_min || !row_max) {
    set_error("pgp_image_rows_needed: bad argument");
    return PGP_EINVAL;
  }
  int lo = -1, hi = -1;
  for (int i = 0; i < n; ++i) {
    int row = 0, col = 0;
    if (!image_pixel(P + 3 * (size_t)i, cP, K, rows, cols, &row, &col)) continue;
    lo = lo < 0 || row < lo ? row : lo;
    hi = row > hi ? row : hi;
  }
  *row_min = lo;
  *row_max = hi;
  return PGP_OK;
}

int pgp_set_scene(pgp_ctx* ctx, const float* xyz, const float* nrm, const float* weight, int n,
                  float delta) {
  if (!ctx || n < 0 || (n > 0 && !xyz) || !(delta > 0.f) || !std::isfinite(delta)) {
    set_error("pgp_set_scene: bad argument (n=%d, delta=%g)", n, (double)delta);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);   // (*_device calls still queued on a caller's stream read the arrays replaced below: the guard drains them)
  // What else can still touch those arrays: the PREVIOUS scene's index build on the side stream (it reads the points) -- the
  // uploads below are ordered behind it on the context's stream, where everything else that rewrites the scene is queued
  // anyway.  (Up to round 5 an unconditional hipDeviceSynchronize stood here; behind a call that returned on its completion
  // word -- the drop-in's last step -- it waited ~30 us for a kernel that had long made its last access to retire.)
  static const bool sync_always = getenv("PGP_SET_SCENE_SYNC") && atoi(getenv("PGP_SET_SCENE_SYNC")) != 0;
  if (sync_always) PGP_HIP(hipDeviceSynchronize());
  else if (ctx->index_pending && ctx->ev_index && !ctx->deferred_build) PGP_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_index, 0));
  ctx->has_index = false;
  ctx->prob_cdf_valid = false;
  ctx->nP = n;
  ctx->has_scene_normals = nrm != nullptr;
  ctx->has_scene_colors = false;
  // packed {x, y, z, id} / {nx, ny, nz, w}: through a pinned staging buffer of this call's own for scenes up to 4 MB (the
  // uploads are then queued and nobody waits for them here: an event tells the side-stream index build when they are
  // through), through temporaries and a synchronisation beyond
  const size_t N = (size_t)std::max(n, 1), bytes = N * sizeof(float4);
  const bool staged = 2 * bytes <= ((size_t)4 << 20);
  std::vector<float4> tmp;
  float4 *hp, *hn;
  int rc;
  if (staged) {
    if (ctx->ev_s) PGP_HIP(hipEventSynchronize(ctx->ev_s));   // the previous scene's copies out of the staging buffer
    else PGP_HIP(hipEventCreateWithFlags(&ctx->ev_s, hipEventDisableTiming));
    if ((rc = ctx->h_s_pin.ensure(2 * bytes)) != PGP_OK) return rc;
    hp = ctx->h_s_pin.as<float4>();
    hn = hp + N;
  } else {
    tmp.resize(2 * N);
    hp = tmp.data();
    hn = hp + N;
  }
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    hp[i] = make_float4(p[0], p[1], p[2], __builtin_bit_cast(float, i));
    float w = weight ? weight[i] : 1.0f;
    if (nrm)
      hn[i] = make_float4(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], w);
    else
      hn[i] = make_float4(0.f, 0.f, 0.f, w);
  }
  if ((rc = ctx->d_P.ensure(bytes)) != PGP_OK) return rc;
  if ((rc = ctx->d_Pnw.ensure(bytes)) != PGP_OK) return rc;
  if (staged) {   // (out of the pinned image: by a kernel on the stream, no copy-engine hand-over in front of the next launch)
    if ((rc = stage_to_device(ctx->stream, ctx->d_P.p, hp, (size_t)n * sizeof(float4))) != PGP_OK) return rc;
    if ((rc = stage_to_device(ctx->stream, ctx->d_Pnw.p, hn, (size_t)n * sizeof(float4))) != PGP_OK) return rc;
  } else {
    PGP_HIP(hipMemcpyAsync(ctx->d_P.p, hp, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    PGP_HIP(hipMemcpyAsync(ctx->d_Pnw.p, hn, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  }
  ctx->scene_upload_pending = false;
  if (staged) {
    PGP_HIP(hipEventRecord(ctx->ev_s, ctx->stream));
    ctx->scene_upload_pending = true;
  } else {
    PGP_HIP(hipStreamSynchronize(ctx->stream));
  }
  ctx->kd_valid = false;
  if (ctx->exact_ties && (rc = build_kd_ties(ctx, xyz, n)) != PGP_OK) return rc;
  return build_index(ctx, xyz, delta);
}

int pgp_set_scene_weights(pgp_ctx* ctx, const float* weight, int n) {
  if (!ctx || n < 0 || (n > 0 && !weight)) {
    set_error("pgp_set_scene_weights: bad argument");
    return PGP_EINVAL;
  }
  if (n != ctx->nP) {
    set_error("pgp_set_scene_weights: %d weights for a scene of %d points", n, ctx->nP);
    return PGP_ESTATE;
  }
  if (n == 0) return PGP_OK;
  if (!ctx->has_index) {
    set_error("pgp_set_scene_weights: no scene (pgp_set_scene first)");
    return PGP_ESTATE;
  }
  // a pgp_score_lcp_device / pgp_settle_records_device call still queued on the caller's stream reads these weights:
  // the guard drains the device when such a call has been noted (note_device_work).  Not unconditionally: an index
  // build still running on the context's side stream (small scenes) reads the points only, and the caller's next
  // steps -- base selection, congruent sets -- are meant to run beside it.
  CtxGuard guard(ctx);
  int rc = ctx->d_pre_io.ensure((size_t)n * 4);
  if (rc != PGP_OK) return rc;
  if ((rc = ctx->d_prob_cdf.ensure((size_t)n * 8)) != PGP_OK) return rc;
  // The weights and -- base selection draws its first point from them -- their double prefix sums (the sequence
  // launch_select_bases would otherwise read back and add up on its first call) go up from a pinned staging buffer of
  // this call's own: nothing of the caller's is read after the return, and nothing waits for the copies here (the
  // caller's next step, the base selection, queues behind them on the stream).
  const size_t off_cdf = ((size_t)n * 4 + 63) & ~(size_t)63, need = off_cdf + (size_t)n * 8;
  if (ctx->ev_w) PGP_HIP(hipEventSynchronize(ctx->ev_w));   // the previous call's copies out of the staging buffer
  else PGP_HIP(hipEventCreateWithFlags(&ctx->ev_w, hipEventDisableTiming));
  if ((rc = ctx->h_w_pin.ensure(need)) != PGP_OK) return rc;
  unsigned char* pin = ctx->h_w_pin.as<unsigned char>();
  std::memcpy(pin, weight, (size_t)n * 4);
  double* cdf = reinterpret_cast<double*>(pin + off_cdf);
  double run = 0.0;
  for (int i = 0; i < n; ++i) {
    run += (double)weight[i];
    cdf[i] = run;
  }
  ctx->prob_cdf_valid = false;
  if ((rc = stage_to_device(ctx->stream, ctx->d_pre_io.p, pin, (size_t)n * 4)) != PGP_OK) return rc;
  if ((rc = launch_scene_weights(ctx, ctx->d_pre_io.as<float>(), n, ctx->stream)) != PGP_OK) return rc;
  if ((rc = stage_to_device(ctx->stream, ctx->d_prob_cdf.p, cdf, (size_t)n * 8)) != PGP_OK) return rc;
  PGP_HIP(hipEventRecord(ctx->ev_w, ctx->stream));
  ctx->prob_cdf_valid = true;
  return PGP_OK;
}

int pgp_set_model(pgp_ctx* ctx, const float* xyz, const float* nrm, int n) {
  if (!ctx || n < 0 || (n > 0 && !xyz)) {
    set_error("pgp_set_model: bad argument (n=%d)", n);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  PGP_HIP(hipDeviceSynchronize());   // see pgp_set_scene
  ctx->nQ = n;
  ctx->has_model_normals = nrm != nullptr;
  // Morton order: neighbouring lanes hold neighbouring model points, so under any rigid
  // transform a wave's 64 queries fall into neighbouring cells (coalesced bitmap / offset /
  // candidate reads, similar run lengths => little divergence).  Scores are sums over the
  // model, so the order is free; q.w keeps the original index for pgp_registered.
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      float v = xyz[3 * (size_t)i + k];
      if (std::isfinite(v)) {
        mn[k] = std::min(mn[k], v);
        mx[k] = std::max(mx[k], v);
      }
    }
  float scale[3];
  for (int k = 0; k < 3; ++k) scale[k] = (mx[k] > mn[k]) ? 1023.0f / (mx[k] - mn[k]) : 0.f;
  std::vector<uint32_t> code((size_t)std::max(n, 1));
  for (int i = 0; i < n; ++i) {
    uint32_t c[3];
    for (int k = 0; k < 3; ++k) {
      float v = (xyz[3 * (size_t)i + k] - mn[k]) * scale[k];
      c[k] = std::isfinite(v) ? (uint32_t)std::min(1023.f, std::max(0.f, v)) : 0u;
    }
    code[i] = spread10(c[0]) | (spread10(c[1]) << 1) | (spread10(c[2]) << 2);
  }
  std::vector<int> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return code[a] != code[b] ? code[a] < code[b] : a < b; });
  std::vector<float4> hq((size_t)std::max(n, 1)), hn((size_t)std::max(n, 1));
  for (int s = 0; s < n; ++s) {
    int i = order[s];
    hq[s] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2],
                        __builtin_bit_cast(float, i));
    hn[s] = nrm ? make_float4(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], 0.f)
                : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  int rc;
  if ((rc = ctx->d_Q.ensure(hq.size() * sizeof(float4))) != PGP_OK) return rc;
  if ((rc = ctx->d_Qn.ensure(hn.size() * sizeof(float4))) != PGP_OK) return rc;
  if ((rc = ctx->d_Qpos.ensure(hq.size() * sizeof(int))) != PGP_OK) return rc;
  std::vector<int> hpos((size_t)std::max(n, 1), 0);
  for (int s = 0; s < n; ++s) hpos[order[s]] = s;
  if ((rc = ctx->d_hits.ensure(hq.size() * sizeof(int))) != PGP_OK) return rc;
  if ((rc = ctx->d_seq.ensure(4 * (hq.size() + 4) * sizeof(float))) != PGP_OK) return rc;  // kRefineGroup rows
  if (ctx->exact_records && (rc = ctx->d_rec_ws.ensure((size_t)records_workspace_bytes(n))) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(ctx->d_Q.p, hq.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  PGP_HIP(hipMemcpyAsync(ctx->d_Qn.p, hn.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  PGP_HIP(hipMemcpyAsync(ctx->d_Qpos.p, hpos.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  // the per-tile partial buffer depends on the model size
  if (ctx->cap_h > 0) {
    int cap = ctx->cap_h;
    ctx->cap_h = 0;
    return pgp_reserve(ctx, cap);
  }
  return PGP_OK;
}

static int reserve_impl(pgp_ctx* ctx, int max_hypotheses);

}  // extern "C"

namespace pgp {
namespace {
// n16 16-byte vectors, then n_tail (< 4) words
__global__ __launch_bounds__(256) void stage_from_host(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16, int n_tail) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) dst[i] = src[i];
  else if (i < n16 + (size_t)n_tail)
    reinterpret_cast<uint32_t*>(dst + n16)[i - n16] = reinterpret_cast<const uint32_t*>(src + n16)[i - n16];
}

struct PubArgs {
  const uint32_t* src[kPubMaxItems];
  uint32_t* dst[kPubMaxItems];
  uint32_t words[kPubMaxItems];
  int n;
  unsigned int* flag;
  unsigned int value;
  unsigned int* ticket;   // device word, zero between launches: the workgroup that draws the last number writes the flag
};
// The items word by word into host memory (system-scope stores: written through, acknowledged), then the word the host polls.
// One workgroup per ~32 KB (up to 32): every workgroup's stores are complete before it draws its ticket, the last one writes
// the word and puts the ticket back.
__global__ __launch_bounds__(1024) void publish_items(PubArgs p) {
  const uint32_t t0 = blockIdx.x * 1024u + threadIdx.x, step = gridDim.x * 1024u;
  for (int k = 0; k < p.n; ++k) {
    const uint32_t* __restrict__ s = p.src[k];
    uint32_t* d = p.dst[k];
    const uint32_t nw = p.words[k];
    if ((((uintptr_t)s | (uintptr_t)d) & 7u) == 0) {   // two words per store
      const unsigned long long* __restrict__ s2 = reinterpret_cast<const unsigned long long*>(s);
      unsigned long long* d2 = reinterpret_cast<unsigned long long*>(d);
      for (uint32_t i = t0; i < nw / 2; i += step) __hip_atomic_store(&d2[i], s2[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if ((nw & 1u) && t0 == 0) __hip_atomic_store(&d[nw - 1], s[nw - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      for (uint32_t i = t0; i < nw; i += step) __hip_atomic_store(&d[i], s[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    bool last = gridDim.x == 1;
    if (!last) {
      last = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
      if (last) __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (last) __hip_atomic_store(p.flag, p.value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace

bool publish_usable(const PubItem* items, int n) {
  static const bool off = getenv("PGP_HOSTOUT_KERNEL") && atoi(getenv("PGP_HOSTOUT_KERNEL")) == 0;
  if (off || n <= 0 || n > kPubMaxItems) return false;
  size_t total = 0;
  for (int k = 0; k < n; ++k) {
    if (((reinterpret_cast<uintptr_t>(items[k].d_src) | reinterpret_cast<uintptr_t>(items[k].h_dst) | items[k].bytes) & 3u) != 0) return false;
    total += items[k].bytes;
  }
  return total <= kPubMaxBytes;
}

// Queues the publishing kernel behind whatever `st` holds and waits for its completion word.  The word is the context's
// (one wait at a time per context); a wait that runs past a generous bound falls back to the stream itself.
int publish_and_wait(pgp_ctx* ctx, hipStream_t st, const PubItem* items, int n) {
  if (!ctx->h_flag) {
    PGP_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_flag), 64, hipHostMallocDefault));
    *ctx->h_flag = 0u;
  }
  PubArgs a{};
  a.n = n;
  for (int k = 0; k < n; ++k) {
    a.src[k] = static_cast<const uint32_t*>(items[k].d_src);
    a.dst[k] = static_cast<uint32_t*>(items[k].h_dst);
    a.words[k] = (uint32_t)(items[k].bytes / 4);
  }
  a.flag = ctx->h_flag;
  a.value = ++ctx->flag_seq ? ctx->flag_seq : ++ctx->flag_seq;
  size_t total = 0;
  for (int k = 0; k < n; ++k) total += items[k].bytes;
  const unsigned groups = (unsigned)std::min<size_t>(32, std::max<size_t>(1, (total + (32u << 10) - 1) / (32u << 10)));
  if (groups > 1) {
    if (!ctx->d_pub_ticket.p) {
      int rc = ctx->d_pub_ticket.ensure(64);
      if (rc != PGP_OK) return rc;
      PGP_HIP(hipMemsetAsync(ctx->d_pub_ticket.p, 0, 64, st));
    }
    a.ticket = ctx->d_pub_ticket.as<unsigned int>();
  }
  hipLaunchKernelGGL(publish_items, dim3(groups), dim3(1024), 0, st, a);
  PGP_HIP(hipGetLastError());
  const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(250);
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(ctx->h_flag, __ATOMIC_ACQUIRE) == a.value) {
      return PGP_OK;
    }
    __builtin_ia32_pause();
    if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() >= t_end) break;
  }
  PGP_HIP(hipStreamSynchronize(st));
  if (__atomic_load_n(ctx->h_flag, __ATOMIC_ACQUIRE) != a.value) {
    set_error("publish_and_wait: the stream finished without the completion word");
    return PGP_EHIP;
  }
  return PGP_OK;
}

// Small inputs on their way from a PINNED host image to the device, fetched by a KERNEL on the stream that is about to use
// them instead of a copy-engine transfer in front of that stream's kernels: the hand-over from the copy engine to the compute
// queue costs ~15 us whatever the size (tools/per_call_probe.py: the 4096-hypothesis host-pointer call 140 -> 126 us, the
// 1024-hypothesis one 70 -> 55 us; profiles/r06_ab/stage_kernel.log), a kernel behind a kernel ~2.5 us.  Up to 2 MB (a
// kernel reads host memory at PCIe speed like the engine does, but occupies compute units while it waits); beyond that,
// unaligned, or with PGP_STAGE_KERNEL=0: hipMemcpyAsync as before.
int stage_to_device(hipStream_t st, void* d_dst, const void* h_pinned, size_t bytes) {
  if (bytes == 0) return PGP_OK;
  static const bool off = getenv("PGP_STAGE_KERNEL") && atoi(getenv("PGP_STAGE_KERNEL")) == 0;
  const bool aligned = ((reinterpret_cast<uintptr_t>(d_dst) | reinterpret_cast<uintptr_t>(h_pinned)) & 15u) == 0 && (bytes & 3u) == 0;
  if (off || !aligned || bytes > (2u << 20)) {
    PGP_HIP(hipMemcpyAsync(d_dst, h_pinned, bytes, hipMemcpyHostToDevice, st));
    return PGP_OK;
  }
  const size_t n16 = bytes / 16;
  const int n_tail = (int)((bytes & 15u) / 4);
  hipLaunchKernelGGL(stage_from_host, dim3((unsigned)((n16 + (size_t)n_tail + 255) / 256)), dim3(256), 0, st,
                     static_cast<const uint4*>(h_pinned), static_cast<uint4*>(d_dst), n16, n_tail);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}
}  // namespace pgp

extern "C" {

int pgp_reserve(pgp_ctx* ctx, int max_hypotheses) {
  if (!ctx || max_hypotheses < 0) {
    set_error("pgp_reserve: bad argument");
    return PGP_EINVAL;
  }
  return reserve_impl(ctx, max_hypotheses);
}

static int reserve_impl(pgp_ctx* ctx, int max_hypotheses) {
  CtxGuard guard(ctx);
  if (int rc = flush_deferred_build(ctx)) return rc;
  if (ctx->index_pending && hipEventQuery(ctx->ev_index) == hipSuccess) {
    const int rc = finish_index(ctx);   // a finished side-stream build: noticed without waiting
    if (rc != PGP_OK) return rc;
  } else if (ctx->index_pending) {
    (void)hipGetLastError();   // hipErrorNotReady is not an error
  }
  if (max_hypotheses <= ctx->cap_h) return PGP_OK;
  PGP_HIP(hipDeviceSynchronize());   // the workspaces replaced below may be in use by queued launches
  if (int rc = index_settled(ctx)) return rc;
  int rc;
  size_t cap = (size_t)max_hypotheses;
  size_t tiles = (size_t)tiles_for(ctx->nQ);
  if ((rc = ctx->d_T.ensure(cap * 16 * sizeof(float))) != PGP_OK) return rc;
  // one row per WAVE of the model: four per tile (lcp_score.hip partial_row)
  if ((rc = ctx->d_partial.ensure(4 * tiles * cap * (sizeof(int) + sizeof(float)))) != PGP_OK) return rc;
  if ((rc = ctx->d_scores.ensure(cap * sizeof(float))) != PGP_OK) return rc;
  if ((rc = ctx->d_counts.ensure(cap * sizeof(int))) != PGP_OK) return rc;
  if ((rc = ctx->d_eo_ws.ensure(cap * sizeof(int) + 64)) != PGP_OK) return rc;
  ctx->cap_h = max_hypotheses;
  return PGP_OK;
}

int pgp_score_lcp_device(pgp_ctx* ctx, const float* d_T, int n_h, int mode, float gate_deg,
                         float* d_scores, int* d_counts, int* d_best, void* stream) {
  if (!ctx || n_h < 0 || (n_h > 0 && (!d_T || !d_scores))) {
    set_error("pgp_score_lcp_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  const int rc = launch_score(ctx, d_T, n_h, mode, gate_deg, d_scores, d_counts, d_best,
                              static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_set_exact_ties(pgp_ctx* ctx, int on) {
  if (!ctx) {
    set_error("pgp_set_exact_ties: ctx is NULL");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  ctx->exact_ties = on != 0;
  if (!ctx->exact_ties) ctx->kd_valid = false;   // the next pgp_set_scene builds the tree again if asked to
  return PGP_OK;
}

int pgp_set_nn_pruning(pgp_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) {
    set_error("pgp_set_nn_pruning: bad argument (mode 0, 1 or 2)");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  ctx->nn_mode = mode;   // (0: a twin this scene already has stays as it is, unused -- a graph captured with it may still replay)
  return PGP_OK;
}

int pgp_get_nn_lists_info(pgp_ctx* ctx, int* state, long long* entries_full, long long* entries_kept, long long* lists_emptied,
                          float* pass_ms) {
  if (!ctx) {
    set_error("pgp_get_nn_lists_info: ctx is NULL");
    return PGP_EINVAL;
  }
  DeviceGuard guard(ctx->device);
  const uint2* occ;
  const float4* cand;
  nn_lists(ctx, ctx->stream, &occ, &cand);   // (notices a finished pass)
  const bool twin = ctx->nn_mode != 0 && ctx->nn_state == PGP_NN_LISTS_ADOPTED;
  if (state) *state = ctx->nn_mode != 0 ? ctx->nn_state : PGP_NN_LISTS_FULL;
  if (entries_full) *entries_full = ctx->has_index && !ctx->index_pending ? ctx->n_cand : 0;
  if (entries_kept) *entries_kept = twin ? ctx->nn_kept : 0;
  if (lists_emptied) *lists_emptied = twin ? ctx->nn_emptied : 0;
  if (pass_ms) *pass_ms = twin ? ctx->nn_ms : 0.f;
  return PGP_OK;
}

int pgp_set_exact_records(pgp_ctx* ctx, int on) {
  if (!ctx) {
    set_error("pgp_set_exact_records: ctx is NULL");
    return PGP_EINVAL;
  }
  if (on) {
    CtxGuard guard(ctx);
    int rc = ctx->d_rec_ws.ensure((size_t)records_workspace_bytes(ctx->nQ));
    if (rc != PGP_OK) return rc;
  }
  ctx->exact_records = on != 0;
  return PGP_OK;
}

int pgp_set_verify_early_out(pgp_ctx* ctx, int on) {
  if (!ctx) {
    set_error("pgp_set_verify_early_out: ctx is NULL");
    return PGP_EINVAL;
  }
  ctx->verify_early_out = on != 0;
  return PGP_OK;
}

int pgp_verify_early_out_device(pgp_ctx* ctx, const float* d_T, int n_h, float* d_scores, int* d_counts, void* stream) {
  if (!ctx || n_h < 0 || (n_h > 0 && (!d_T || !d_scores || !d_counts))) {
    set_error("pgp_verify_early_out_device: bad argument");
    return PGP_EINVAL;
  }
  if (n_h > ctx->cap_h) {
    set_error("pgp_verify_early_out_device: %d hypotheses exceed the reserved capacity %d (pgp_reserve)", n_h, ctx->cap_h);
    return PGP_ESTATE;
  }
  CtxGuard guard(ctx, false);
  const int rc = launch_verify_early_out(ctx, d_T, n_h, d_scores, d_counts, static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_settle_records_device(pgp_ctx* ctx, const float* d_T, int n_h, int mode, float gate_deg, float* d_scores,
                              void* stream) {
  if (!ctx || n_h < 0 || (n_h > 0 && (!d_T || !d_scores))) {
    set_error("pgp_settle_records_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  // queue-only entry: no allocation here (a hipFree / hipMalloc would synchronise the device and break a
  // capture); the workspace is reserved by pgp_set_exact_records / pgp_set_model
  if (ctx->d_rec_ws.cap < (size_t)records_workspace_bytes(ctx->nQ)) {
    set_error("pgp_settle_records_device: workspace not reserved (call pgp_set_exact_records(ctx, 1) after pgp_set_model)");
    return PGP_ESTATE;
  }
  int rc = launch_settle_records(ctx, d_T, n_h, mode, gate_deg, d_scores, static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_settle_best_device(pgp_ctx* ctx, const float* d_T, int n_h, int mode, float gate_deg,
                           float* d_scores, int* d_best, void* stream) {
  if (!ctx || n_h < 0 || !d_best || (n_h > 0 && (!d_T || !d_scores))) {
    set_error("pgp_settle_best_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  const int rc = launch_settle_best(ctx, d_T, n_h, mode, gate_deg, d_scores, d_best, static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_score_lcp(pgp_ctx* ctx, const float* T, int n_h, int mode, float gate_deg, float* scores,
                  int* counts, int* best_index, float* best_score) {
  if (!ctx || n_h < 0 || (n_h > 0 && (!T || !scores))) {
    set_error("pgp_score_lcp: bad argument");
    return PGP_EINVAL;
  }
  // PGP_CALL_PHASES=1: where a call's wall time goes, printed to stderr every 100 calls (diagnostic)
  static const bool phases = getenv("PGP_CALL_PHASES") != nullptr;
  static thread_local double ph_acc[8] = {0};
  static thread_local int ph_n = 0;
  double ph_t = 0.0;
  int ph_k = 0;
  auto ph_now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  auto ph_mark = [&] {
    if (!phases) return;
    const double t = ph_now();
    if (ph_k > 0) ph_acc[ph_k - 1] += t - ph_t;
    ph_t = t;
    ++ph_k;
  };
  ph_mark();
  CtxGuard guard(ctx);
  int rc = reserve_impl(ctx, n_h);
  if (rc != PGP_OK) return rc;
  hipStream_t st = ctx->stream;
  ph_mark();   // [0] guard + reserve
  // The caller's arrays are pageable (std::vector storage in the node): copying them through a
  // pinned staging buffer of our own makes the two transfers plain DMA (one H2D, ONE D2H of
  // scores | counts | best) instead of the runtime's chunked pageable path -- 199 -> ~150 us per
  // 4096-hypothesis call.
  const size_t nT = (size_t)n_h * 16 * sizeof(float);
  const size_t out_bytes = (size_t)n_h * 8 + 8;
  const size_t pin_need = nT + out_bytes + 64 + 256;   // + {index, score bits, near, spare} and the completion word
  if ((rc = ctx->h_pin.ensure(pin_need)) != PGP_OK) return rc;
  if ((rc = ctx->d_out.ensure(out_bytes)) != PGP_OK) return rc;
  unsigned char* pin = ctx->h_pin.as<unsigned char>();
  unsigned char* pin_out = pin + ((nT + 63) & ~(size_t)63);
  float* d_scores = ctx->d_out.as<float>();
  int* d_counts = reinterpret_cast<int*>(d_scores + n_h);
  int* d_best = d_counts + n_h;
  if (n_h > 0) {
    std::memcpy(pin, T, nT);
    ph_mark();   // [1] transforms into the pinned image
    if ((rc = stage_to_device(st, ctx->d_T.p, pin, nT)) != PGP_OK) return rc;
    ph_mark();   // [2] H2D queued
  }
  // The results' way back.  finalize_scores writes scores, counts and the best straight into the pinned landing area, and a
  // completion word behind them (lcp_score.hip HostPub): no device-to-host copy (a DMA of its own behind the kernel: ~10 us
  // whatever its size) and no wait for the end-of-kernel signal -- the host polls the word.  The opt-in passes over the score
  // vector (exact records, Verify's early termination), a weighted near-tie settled on the device and PGP_HOST_RESULTS=0
  // copy back as before.
  static const bool host_results = !(getenv("PGP_HOST_RESULTS") && atoi(getenv("PGP_HOST_RESULTS")) == 0);
  unsigned char* pin_tail = pin_out + ((out_bytes + 63) & ~(size_t)63);
  ScoreHostOut ho{};
  ho.scores = reinterpret_cast<float*>(pin_out);
  ho.counts = reinterpret_cast<int*>(pin_out + (size_t)n_h * 4);
  ho.best = reinterpret_cast<int*>(pin_tail);
  ho.flag = reinterpret_cast<unsigned int*>(pin_tail + 64);
  ho.flag_value = ++ctx->flag_seq ? ctx->flag_seq : ++ctx->flag_seq;   // never 0
  const bool want_host = host_results && n_h > 0 && !ctx->exact_records && !(ctx->verify_early_out && mode == PGP_MODE_PLAIN);
  if (want_host) {
    // (the word must not hold this call's value from the area's earlier life: the area is re-allocated when it grows)
    __atomic_store_n(ho.flag, 0u, __ATOMIC_RELAXED);
  }
  rc = launch_score(ctx, ctx->d_T.as<float>(), n_h, mode, gate_deg, d_scores, d_counts, d_best, st, want_host ? &ho : nullptr);
  if (rc != PGP_OK) return rc;
  ph_mark();     // [3] kernels queued
  bool via_host = want_host && ho.published;
  if (via_host) {
    ph_mark();   // [4] (no copy to queue)
    // the kernel's own launch is ~0.1 ms per 4096 hypotheses; past a generous bound the stream is asked instead
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(20 + n_h / 64);
    bool seen = false;
    for (unsigned spins = 0;; ++spins) {
      if (__atomic_load_n(ho.flag, __ATOMIC_ACQUIRE) == ho.flag_value) {
        seen = true;
        break;
      }
      __builtin_ia32_pause();
      if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() >= t_end) break;
    }
    if (!seen) {
      PGP_HIP(hipStreamSynchronize(st));
      if (__atomic_load_n(ho.flag, __ATOMIC_ACQUIRE) != ho.flag_value) {
        set_error("pgp_score_lcp: the scoring launch finished without publishing its results");
        return PGP_EHIP;
      }
    }
    ph_mark();   // [5] the wait
    if (ho.best[2] != 0) via_host = false;   // weighted near-tie (rare): settled on the device, its arrays come the old way
  }
  if (!via_host) {
    PGP_HIP(hipMemcpyAsync(pin_out, d_scores, out_bytes, hipMemcpyDeviceToHost, st));
    ph_mark();     // [4] D2H queued
    PGP_HIP(hipStreamSynchronize(st));
      ph_mark();     // [5] the wait
  }
  if ((rc = index_settled(ctx)) != PGP_OK) return rc;
  if (n_h > 0) {
    std::memcpy(scores, pin_out, (size_t)n_h * sizeof(float));
    if (counts) std::memcpy(counts, pin_out + (size_t)n_h * 4, (size_t)n_h * sizeof(int));
  }
  int best[2];
  std::memcpy(best, via_host ? pin_tail : pin_out + (size_t)n_h * 8, sizeof best);
  if (best_index) *best_index = best[0];
  if (best_score) std::memcpy(best_score, &best[1], 4);
  ph_mark();     // [6] results out of the pinned image
  if (phases && ++ph_n == 100) {
    fprintf(stderr, "pgp_score_lcp phases (us, mean of 100 calls, n_h %d): reserve %.1f | stage T %.1f | queue H2D %.1f | queue kernels %.1f | "
                    "queue D2H %.1f | wait %.1f | copy out %.1f\n", n_h, ph_acc[0] / 100, ph_acc[1] / 100, ph_acc[2] / 100, ph_acc[3] / 100,
            ph_acc[4] / 100, ph_acc[5] / 100, ph_acc[6] / 100);
    for (double& a : ph_acc) a = 0;
    ph_n = 0;
  }
  return PGP_OK;
}

int pgp_registered(pgp_ctx* ctx, const float* T16, int mode, float gate_deg, int* ids, int* n) {
  if (!ctx || !T16 || !n || (ctx->nQ > 0 && !ids)) {
    set_error("pgp_registered: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  int rc = pgp_reserve(ctx, 1);
  if (rc != PGP_OK) return rc;
  hipStream_t st = ctx->stream;
  PGP_HIP(hipMemcpyAsync(ctx->d_T.p, T16, 16 * sizeof(float), hipMemcpyHostToDevice, st));
  rc = launch_registered(ctx, ctx->d_T.as<float>(), mode, gate_deg, ctx->d_hits.as<int>(), st);
  if (rc != PGP_OK) return rc;
  HostOut out(ctx, st);
  const unsigned char* got = nullptr;
  if ((rc = out.fetch(&got, ctx->d_hits.p, (size_t)ctx->nQ * sizeof(int))) != PGP_OK || (rc = out.sync()) != PGP_OK) return rc;
  const int* hits = reinterpret_cast<const int*>(got);
  if ((rc = index_settled(ctx)) != PGP_OK) return rc;
  int k = 0;
  for (int i = 0; i < ctx->nQ; ++i)
    if (hits[i] >= 0) ids[k++] = hits[i];  // model-point order, as push_back in base.cc:1760
  *n = k;
  return PGP_OK;
}

int pgp_registered_model(pgp_ctx* ctx, const float* T16, const float* q_xyz, const float* q_nrm, int n,
                         float gate_deg, int* ids, int* n_ids) {
  if (!ctx || !T16 || !n_ids || n < 0 || (n > 0 && (!q_xyz || !q_nrm || !ids))) {
    set_error("pgp_registered_model: bad argument");
    return PGP_EINVAL;
  }
  *n_ids = 0;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  std::vector<float4> hq((size_t)n), hn((size_t)n);
  for (int i = 0; i < n; ++i) {
    hq[i] = make_float4(q_xyz[3 * (size_t)i], q_xyz[3 * (size_t)i + 1], q_xyz[3 * (size_t)i + 2], 0.f);
    hn[i] = make_float4(q_nrm[3 * (size_t)i], q_nrm[3 * (size_t)i + 1], q_nrm[3 * (size_t)i + 2], 0.f);
  }
  const size_t N = (size_t)n;
  int rc = ctx->d_pre_io.ensure(N * 36 + 64 + 256);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_pre_io.as<unsigned char>();
  float4* d_q = reinterpret_cast<float4*>(base);
  float4* d_n = d_q + N;
  int* d_hits = reinterpret_cast<int*>(d_n + N);
  float* d_T = reinterpret_cast<float*>(d_hits + N);
  d_T = reinterpret_cast<float*>(((uintptr_t)d_T + 63) & ~(uintptr_t)63);
  PGP_HIP(hipMemcpyAsync(d_q, hq.data(), N * 16, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_n, hn.data(), N * 16, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_T, T16, 64, hipMemcpyHostToDevice, st));
  rc = launch_registered_model(ctx, d_T, d_q, d_n, n, gate_deg, d_hits, st);
  if (rc != PGP_OK) return rc;
  HostOut out(ctx, st);
  const unsigned char* got = nullptr;
  if ((rc = out.fetch(&got, d_hits, N * 4)) != PGP_OK || (rc = out.sync()) != PGP_OK) return rc;
  const int* hits = reinterpret_cast<const int*>(got);
  if ((rc = index_settled(ctx)) != PGP_OK) return rc;
  int k = 0;
  for (int i = 0; i < n; ++i)
    if (hits[i] >= 0) ids[k++] = hits[i];
  *n_ids = k;
  return PGP_OK;
}

int pgp_find_congruent_4pcs(pgp_ctx* ctx, float invariant1, float invariant2, float threshold, const int* P_pairs,
                            int nP, const int* Q_pairs, int nQ, int* quads, int cap, int* n_quads) {
  if (!ctx || !n_quads || nP < 0 || nQ < 0 || cap < 0 || (nP > 0 && !P_pairs) || (nQ > 0 && !Q_pairs) ||
      (cap > 0 && !quads)) {
    set_error("pgp_find_congruent_4pcs: bad argument");
    return PGP_EINVAL;
  }
  *n_quads = 0;
  if (nP == 0 || nQ == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = ctx->d_cs_pairs.ensure(((size_t)nP + nQ) * 8)) != PGP_OK) return rc;
  if ((rc = ctx->d_cs_out.ensure((size_t)std::max(cap, 1) * 16)) != PGP_OK) return rc;
  int* d_Pp = ctx->d_cs_pairs.as<int>();
  int* d_Qp = d_Pp + 2 * (size_t)nP;
  PGP_HIP(hipMemcpyAsync(d_Pp, P_pairs, (size_t)nP * 8, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_Qp, Q_pairs, (size_t)nQ * 8, hipMemcpyHostToDevice, st));
  int total = 0;
  rc = launch_find_congruent_4pcs(ctx, invariant1, invariant2, threshold, d_Pp, nP, d_Qp, nQ, ctx->d_cs_out.as<int>(), cap,
                                  &total, st);
  if (rc != PGP_OK) return rc;
  const int n_copy = std::min(total, cap);
  if (n_copy > 0) PGP_HIP(hipMemcpyAsync(quads, ctx->d_cs_out.p, (size_t)n_copy * 16, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  *n_quads = total;
  return PGP_OK;
}

int pgp_running_best(const float* scores, int n_h, int* selected, int* n_selected) {
  if (n_h < 0 || (n_h > 0 && (!scores || !selected)) || !n_selected) {
    set_error("pgp_running_best: bad argument");
    return PGP_EINVAL;
  }
  float best = 0.f;  // best_LCP_ = 0.0 (base.cc:308)
  int k = 0;
  for (int i = 0; i < n_h; ++i)
    if (scores[i] > best) {
      best = scores[i];
      selected[k++] = i;
    }
  *n_selected = k;
  return PGP_OK;
}

int pgp_set_search_model(pgp_ctx* ctx, const float* xyz, int n) {
  if (!ctx || n < 0 || (n > 0 && !xyz)) {
    set_error("pgp_set_search_model: bad argument (n=%d)", n);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  PGP_HIP(hipDeviceSynchronize());   // see pgp_set_scene
  ctx->csb_fit_m = 0;
  ctx->csb_nb = 0;   // a resident congruent batch belongs to the old search model
  ctx->v4_nb = 0;    // and so does a resident V4PCS batch
  ctx->s4_nl = 0;    // and the pair lists of pgp_extract_pairs_batch
  ctx->s4_off.clear();
  ctx->has_search_normals = ctx->has_search_colors = false;   // the attributes belong to the old points
  std::vector<float4> hq((size_t)std::max(n, 1));
  for (int i = 0; i < n; ++i)
    hq[i] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2],
                        __builtin_bit_cast(float, i));
  int rc = ctx->d_Qs.ensure(hq.size() * sizeof(float4));
  if (rc != PGP_OK) return rc;
  // unit-cube image for the congruent-set accelerators (pairCreationFunctor.h:102-138)
  std::vector<float4> hu;
  unit_cube_image(xyz, n, ctx->cs_gcenter, &ctx->cs_ratio, &hu);
  if ((rc = ctx->d_Qs_unit.ensure(hu.size() * sizeof(float4))) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(ctx->d_Qs_unit.p, hu.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  PGP_HIP(hipMemcpyAsync(ctx->d_Qs.p, hq.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  ctx->nQs = n;
  return PGP_OK;
}

int pgp_set_ppf_map(pgp_ctx* ctx, const int* keys, const int* counts, const int* pairs, int n_keys) {
  if (!ctx || n_keys < 0 || (n_keys > 0 && !keys)) {
    set_error("pgp_set_ppf_map: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  PGP_HIP(hipDeviceSynchronize());
  return set_ppf_map(ctx, keys, counts, pairs, n_keys);
}

int pgp_set_ppf_map_from_model(pgp_ctx* ctx, const float* xyz, const float* nrm, int n, int* n_keys, long long* n_pairs) {
  if (!ctx || !xyz || !nrm || n < 2 || n > PGP_PPF_BUILD_MAX_POINTS) {
    set_error("pgp_set_ppf_map_from_model: bad argument (n=%d, 2 .. %d points with normals)", n, PGP_PPF_BUILD_MAX_POINTS);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  PGP_HIP(hipDeviceSynchronize());
  int nk = 0;
  long long np = 0;
  const int rc = build_ppf_map(ctx, xyz, nrm, n, &nk, &np);
  if (rc != PGP_OK) return rc;
  if (n_keys) *n_keys = nk;
  if (n_pairs) *n_pairs = np;
  return PGP_OK;
}

int pgp_get_ppf_map(pgp_ctx* ctx, int* keys, int* counts, int* pairs, int cap_keys, long long cap_pairs, int* n_keys,
                    long long* n_pairs) {
  if (!ctx || cap_keys < 0 || cap_pairs < 0) {
    set_error("pgp_get_ppf_map: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  int nk = 0;
  long long np = 0;
  const int rc = get_ppf_map(ctx, keys, counts, pairs, cap_keys, cap_pairs, &nk, &np);
  if (rc != PGP_OK) return rc;
  if (n_keys) *n_keys = nk;
  if (n_pairs) *n_pairs = np;
  return PGP_OK;
}

int pgp_select_bases(pgp_ctx* ctx, const double* u, int n_attempts, int* ids, float* invariants, int* status) {
  if (!ctx || n_attempts < 0 || (n_attempts > 0 && (!u || !ids || !invariants || !status))) {
    set_error("pgp_select_bases: bad argument");
    return PGP_EINVAL;
  }
  if (n_attempts == 0) return PGP_OK;
  CtxGuard guard(ctx);
  return launch_select_bases(ctx, u, n_attempts, ids, invariants, status, nullptr, ctx->stream);
}

int pgp_select_bases_rows(pgp_ctx* ctx, const double* u, int n_attempts, int* ids, float* invariants, int* status, int* rows) {
  if (!ctx || n_attempts < 0 || (n_attempts > 0 && (!u || !ids || !invariants || !status || !rows))) {
    set_error("pgp_select_bases_rows: bad argument");
    return PGP_EINVAL;
  }
  if (n_attempts == 0) return PGP_OK;
  CtxGuard guard(ctx);
  return launch_select_bases(ctx, u, n_attempts, ids, invariants, status, rows, ctx->stream);
}

int pgp_select_bases_rows_begin(pgp_ctx* ctx, const double* u, int n_attempts) {
  if (!ctx || n_attempts <= 0 || !u) {
    set_error("pgp_select_bases_rows_begin: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_select_bases(ctx, u, n_attempts, nullptr, nullptr, nullptr, nullptr, ctx->stream, 1);
}

int pgp_select_bases_rows_end(pgp_ctx* ctx, int* ids, float* invariants, int* status, int* rows) {
  if (!ctx || !ids || !invariants || !status) {
    set_error("pgp_select_bases_rows_end: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_select_bases(ctx, nullptr, 0, ids, invariants, status, rows, ctx->stream, 2);
}

int pgp_ppf_features(pgp_ctx* ctx, const int* pairs, int m, int* features, int* rows) {
  if (!ctx || m < 0 || (m > 0 && (!pairs || !features))) {
    set_error("pgp_ppf_features: bad argument");
    return PGP_EINVAL;
  }
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  return launch_ppf_features(ctx, pairs, m, features, rows, ctx->stream);
}

int pgp_stocs_stage_weights(pgp_ctx* ctx, int stage, int base1, int base2, int base3, float* cur, float* sum,
                            int* present) {
  if (!ctx || !cur || !sum || !present) {
    set_error("pgp_stocs_stage_weights: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_stage_weights(ctx, stage, base1, base2, base3, cur, sum, present, ctx->stream);
}

int pgp_base_invariants(pgp_ctx* ctx, int* ids, int m, float* invariants, int* ok) {
  if (!ctx || m < 0 || (m > 0 && (!ids || !invariants || !ok))) {
    set_error("pgp_base_invariants: bad argument");
    return PGP_EINVAL;
  }
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  return launch_base_invariants(ctx, ids, m, invariants, ok, ctx->stream);
}

int pgp_rigid_from_congruent_device(pgp_ctx* ctx, const int* d_base_ids, const int* d_quad_ids, int n,
                                    const float centroid_P[3], const float centroid_Q[3], float* d_T,
                                    double* d_pose, int* d_status, float* d_rms, void* stream) {
  if (!ctx || n < 0 || !centroid_P || !centroid_Q || (n > 0 && (!d_base_ids || !d_quad_ids || !d_T || !d_status))) {
    set_error("pgp_rigid_from_congruent_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  const int rc = launch_rigid(ctx, d_base_ids, d_quad_ids, n, centroid_P, centroid_Q, d_T, d_pose, d_status, d_rms,
                              static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_rigid_from_congruent(pgp_ctx* ctx, const int* base_ids, const int* quad_ids, int n,
                             const float centroid_P[3], const float centroid_Q[3], float* T,
                             double* pose, int* status, float* rms) {
  if (!ctx || n < 0 || !centroid_P || !centroid_Q || (n > 0 && (!base_ids || !quad_ids || !T || !status))) {
    set_error("pgp_rigid_from_congruent: bad argument");
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)n;
  int rc;
  if ((rc = ctx->d_ids.ensure(N * 32)) != PGP_OK) return rc;
  ctx->csb_fit_m = 0;   // d_rig is rewritten below: the fits a pgp_congruent_batch_fetch could name are gone
  if ((rc = ctx->d_rig.ensure(rig_fits(ctx, N).bytes)) != PGP_OK) return rc;
  int* d_b = ctx->d_ids.as<int>();
  int* d_q = d_b + 4 * N;
  const RigFits fit = rig_fits(ctx, N);
  PGP_HIP(hipMemcpyAsync(d_b, base_ids, N * 16, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_q, quad_ids, N * 16, hipMemcpyHostToDevice, st));
  rc = launch_rigid(ctx, d_b, d_q, n, centroid_P, centroid_Q, fit.T, fit.pose, fit.status, fit.rms, st);
  if (rc != PGP_OK) return rc;
  return fits_home(ctx, fit, N, T, pose, status, rms, st);
}

int pgp_extract_pairs(pgp_ctx* ctx, float pair_distance, float eps, int* pairs, int cap, int* n_pairs) {
  if (!ctx || !n_pairs || cap < 0 || (cap > 0 && !pairs) || !(eps >= 0.f)) {
    set_error("pgp_extract_pairs: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  int rc = ctx->d_cs_out.ensure((size_t)std::max(cap, 1) * 8);
  if (rc != PGP_OK) return rc;
  int total = 0;
  rc = launch_extract_pairs(ctx, pair_distance, eps, ctx->d_cs_out.as<int>(), cap, &total, st);
  if (rc != PGP_OK) return rc;
  int n_copy = std::min(total, cap);
  if (n_copy > 0)
    PGP_HIP(hipMemcpyAsync(pairs, ctx->d_cs_out.p, (size_t)n_copy * 8, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  *n_pairs = total;
  return PGP_OK;
}

int pgp_find_congruent(pgp_ctx* ctx, const float* base, float invariant1, float invariant2, float threshold,
                       const int* P_pairs, int nP, const int* Q_pairs, int nQ, int* quads, int cap,
                       int* n_quads) {
  if (!ctx || !base || !n_quads || nP < 0 || nQ < 0 || cap < 0 || (nP > 0 && !P_pairs) ||
      (nQ > 0 && !Q_pairs) || (cap > 0 && !quads)) {
    set_error("pgp_find_congruent: bad argument");
    return PGP_EINVAL;
  }
  *n_quads = 0;
  if (nP == 0 || nQ == 0) return PGP_OK;
  if (nP >= (1 << 24) || nQ >= (1 << 24)) {   // the join's keys hold a pair index in 24 bits; refused before any upload
    set_error("pgp_find_congruent: a pair list exceeds 2^24 entries");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = ctx->d_cs_pairs.ensure(((size_t)nP + nQ) * 8)) != PGP_OK) return rc;
  if ((rc = ctx->d_cs_out.ensure((size_t)std::max(cap, 1) * 16)) != PGP_OK) return rc;
  int2* d_pairs = ctx->d_cs_pairs.as<int2>();   // P_pairs | Q_pairs
  PGP_HIP(hipMemcpyAsync(d_pairs, P_pairs, (size_t)nP * 8, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_pairs + nP, Q_pairs, (size_t)nQ * 8, hipMemcpyHostToDevice, st));
  int total = 0;
  rc = launch_find_congruent(ctx, base, invariant1, invariant2, threshold, d_pairs, nP, nQ, ctx->d_cs_out.as<int4>(), cap,
                             &total, st);
  if (rc != PGP_OK) return rc;
  int n_copy = std::min(total, cap);
  if (n_copy > 0)
    PGP_HIP(hipMemcpyAsync(quads, ctx->d_cs_out.p, (size_t)n_copy * 16, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  *n_quads = total;
  return PGP_OK;
}

int pgp_find_congruent_batch(pgp_ctx* ctx, const int* base_ids, const float* base_xyz, const float* invariants,
                             int n_bases, float threshold, int* n_quads) {
  if (!ctx || n_bases < 0 || (n_bases > 0 && (!base_ids || !base_xyz || !invariants || !n_quads))) {
    set_error("pgp_find_congruent_batch: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_find_congruent_batch(ctx, base_ids, base_xyz, invariants, nullptr, n_bases, threshold, n_quads, ctx->stream);
}

int pgp_find_congruent_batch_rows(pgp_ctx* ctx, const int* base_ids, const float* base_xyz, const float* invariants,
                                  const int* rows, int n_bases, float threshold, int* n_quads) {
  if (!ctx || n_bases < 0 || (n_bases > 0 && (!base_ids || !base_xyz || !invariants || !rows || !n_quads))) {
    set_error("pgp_find_congruent_batch_rows: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_find_congruent_batch(ctx, base_ids, base_xyz, invariants, rows, n_bases, threshold, n_quads, ctx->stream);
}

int pgp_congruent_batch_quads(pgp_ctx* ctx, const int* picks, int m, int* quads) {
  if (!ctx || m < 0 || (m > 0 && (!picks || !quads))) {
    set_error("pgp_congruent_batch_quads: bad argument");
    return PGP_EINVAL;
  }
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  int rc = ctx->d_cs_out.ensure((size_t)m * 16);
  if (rc != PGP_OK) return rc;
  rc = launch_congruent_batch_gather(ctx, picks, m, ctx->d_cs_out.as<int4>(), ctx->stream);
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(quads, ctx->d_cs_out.p, (size_t)m * 16, hipMemcpyDeviceToHost, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  return PGP_OK;
}

int pgp_congruent_batch_fit(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                            const float centroid_Q[3], float* T, double* pose, int* status, float* rms) {
  if (!ctx || m < 0 || !centroid_P || !centroid_Q || (m > 0 && (!picks || !base_ids || !T || !status))) {
    set_error("pgp_congruent_batch_fit: bad argument");
    return PGP_EINVAL;
  }
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)m;
  int rc;
  if ((rc = ctx->d_ids.ensure(N * 32)) != PGP_OK) return rc;
  ctx->csb_fit_m = 0;   // d_rig is rewritten below: the fits a pgp_congruent_batch_fetch could name are gone
  if ((rc = ctx->d_rig.ensure(rig_fits(ctx, N).bytes)) != PGP_OK) return rc;
  int* d_b = ctx->d_ids.as<int>();
  int* d_q = d_b + 4 * N;
  // the base of every pick (scene ids), staged from the host; the quads never leave the device
  std::vector<int> hb(4 * N);
  if (!pick_bases(picks, N, base_ids, hb.data(), ctx->csb_nb, "pgp_congruent_batch_fit")) return PGP_EINVAL;
  PGP_HIP(hipMemcpyAsync(d_b, hb.data(), N * 16, hipMemcpyHostToDevice, st));
  rc = launch_congruent_batch_gather(ctx, picks, m, reinterpret_cast<int4*>(d_q), st);
  if (rc != PGP_OK) return rc;
  const RigFits fit = rig_fits(ctx, N);
  rc = launch_rigid(ctx, d_b, d_q, m, centroid_P, centroid_Q, fit.T, fit.pose, fit.status, fit.rms, st);
  if (rc != PGP_OK) return rc;
  return fits_home(ctx, fit, N, T, pose, status, rms, st);   // (hb, the pageable staging vector, lives until the wait is over)
}

namespace {
// a fit the reference does not push (status != 1: base.cc:1467-1485) is replaced by a transform that registers
// nothing -- identity rotation, translation 1e6 -- so that it scores 0 and can never enter the running-best walk
__global__ __launch_bounds__(256) void mask_failed_fits(const int* __restrict__ status, int m, float* __restrict__ T) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || status[i] == 1) return;
  float* o = T + 16 * (size_t)i;
  for (int q = 0; q < 16; ++q) o[q] = (q % 5 == 0) ? 1.f : 0.f;
  o[12] = o[13] = o[14] = 1e6f;
}
// 16 lanes per kept fit: its float transform and its double pose into a contiguous staging block
__global__ __launch_bounds__(64) void gather_fits(const int* __restrict__ index, int k, const float* __restrict__ T,
                                                  const double* __restrict__ pose, float* __restrict__ T_out,
                                                  double* __restrict__ pose_out) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 4), q = threadIdx.x & 15;
  if (j >= k) return;
  const size_t h = (size_t)index[j];
  T_out[16 * (size_t)j + q] = T[16 * h + q];
  pose_out[16 * (size_t)j + q] = pose[16 * h + q];
}

// The running-best walk of the verification loop (base.cc:1891-1908: hypothesis i enters when lcp_i > best so far, strict,
// best_LCP_ = 0 to begin with) over the FINAL scores on the device -- what pgp_running_best does on the host, entry for
// entry.  One block; 16 consecutive scores per thread, the running maximum in front of a thread's run by a prefix-max over
// the block.  list[0] = number of records (all of them), list[1] = number of fits that were pushed (status == 1),
// list[2 .. 2 + cap) = the first cap records' indices, rec_score[cap] their scores.
__global__ __launch_bounds__(256) void records_walk(int n, const float* __restrict__ scores, const int* __restrict__ status, int cap,
                                                    int* __restrict__ list, float* __restrict__ rec_score) {
  constexpr int kPer = 16;
  __shared__ float s_wmax[4];
  __shared__ int s_wcnt[4], s_wkept[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float carry = 0.f;
  int base = 0, kept = 0;
  for (int s0 = 0; s0 < n; s0 += 256 * kPer) {
    float v[kPer];
    const int lo = s0 + tid * kPer;
    int my_kept = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      v[k] = lo + k < n ? scores[lo + k] : 0.f;
      my_kept += (lo + k < n && status[lo + k] == 1) ? 1 : 0;
    }
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < kPer; ++k) m = fmaxf(m, v[k]);
    // the running maximum in front of this thread's run: prefix-max over the wave, the waves in front, the passes in front
    const float inc = wave::scan_incl(m, lane, wave::Max{});
    float excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 0.f;
    const int ik = wave::scan_incl(my_kept, lane);
    if (lane == 63) s_wkept[wave] = ik;
    wave::block4_publish(s_wmax, lane == 63, inc);
    float run = wave::block4_offset(s_wmax, wave, fmaxf(carry, excl), wave::Max{});
    unsigned mask = 0u;
    int c = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (v[k] > run) {
        run = v[k];
        mask |= 1u << k;
        ++c;
      }
    // where this thread's records go: exclusive count over the wave, the waves in front, the passes in front
    const int ic = wave::scan_incl(c, lane);
    wave::block4_publish(s_wcnt, lane == 63, ic);
    int at = wave::block4_offset(s_wcnt, wave, base + ic - c);
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (mask & (1u << k)) {
        if (at < cap) {
          list[2 + at] = lo + k;
          rec_score[at] = v[k];
        }
        ++at;
      }
    base += wave::block4_total(s_wcnt);
    kept += wave::block4_total(s_wkept);
    carry = fmaxf(carry, wave::block4_total(s_wmax, wave::Max{}));   // (a maximum: the same whatever the order)
    __syncthreads();   // s_wmax / s_wcnt / s_wkept are rewritten by the next pass
  }
  if (tid == 0) {
    list[0] = base;
    list[1] = kept;
  }
}

// entries 0 .. min(records, cap) - 1: the records of `list`; entry cap: the best hypothesis (best[0] < 0: zeros)
__global__ __launch_bounds__(64) void gather_fits_list(const int* __restrict__ list, int cap, const int* __restrict__ best,
                                                       const float* __restrict__ T, const double* __restrict__ pose,
                                                       float* __restrict__ T_out, double* __restrict__ pose_out) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 4), q = threadIdx.x & 15;
  if (j > cap) return;
  const int n_rec = list[0] < cap ? list[0] : cap;
  int h = -1;
  if (j < n_rec) h = list[2 + j];
  else if (j == cap) h = best[0];
  T_out[16 * (size_t)j + q] = h >= 0 ? T[16 * (size_t)h + q] : 0.f;
  pose_out[16 * (size_t)j + q] = h >= 0 ? pose[16 * (size_t)h + q] : 0.0;
}
}  // namespace

int pgp_congruent_batch_fit_score(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                                  const float centroid_Q[3], int mode, float gate_deg, float* scores, int* status,
                                  int* best_index, float* best_score) {
  if (!ctx || m < 0 || !centroid_P || !centroid_Q || (m > 0 && (!picks || !base_ids || !scores || !status))) {
    set_error("pgp_congruent_batch_fit_score: bad argument");
    return PGP_EINVAL;
  }
  if (best_index) *best_index = -1;
  if (best_score) *best_score = 0.f;
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)m;
  int rc;
  if ((rc = pgp_reserve(ctx, m)) != PGP_OK) return rc;
  if ((rc = ctx->d_ids.ensure(N * 32)) != PGP_OK) return rc;
  ctx->csb_fit_m = 0;   // d_rig is rewritten below: the fits a pgp_congruent_batch_fetch could name are gone
  if ((rc = ctx->d_rig.ensure(rig_fits(ctx, N).bytes)) != PGP_OK) return rc;
  if ((rc = ctx->d_out.ensure(N * 8 + 8)) != PGP_OK) return rc;
  // pinned staging: [bases of the picks | picks] in, [scores | status | best] out
  const size_t in_bytes = N * 16, out_bytes = N * 8 + 8;
  if ((rc = ctx->h_pin.ensure(in_bytes + out_bytes + 128)) != PGP_OK) return rc;
  unsigned char* pin = ctx->h_pin.as<unsigned char>();
  int* hb = reinterpret_cast<int*>(pin);
  if (!pick_bases(picks, N, base_ids, hb, ctx->csb_nb, "pgp_congruent_batch_fit_score")) return PGP_EINVAL;
  int* d_b = ctx->d_ids.as<int>();
  int* d_q = d_b + 4 * N;
  PGP_HIP(hipMemcpyAsync(d_b, hb, in_bytes, hipMemcpyHostToDevice, st));
  rc = launch_congruent_batch_gather(ctx, picks, m, reinterpret_cast<int4*>(d_q), st);
  if (rc != PGP_OK) return rc;
  const RigFits fit = rig_fits(ctx, N);
  rc = launch_rigid(ctx, d_b, d_q, m, centroid_P, centroid_Q, fit.T, fit.pose, fit.status, fit.rms, st);
  if (rc != PGP_OK) return rc;
  hipLaunchKernelGGL(mask_failed_fits, dim3((m + 255) / 256), dim3(256), 0, st, (const int*)fit.status, m, fit.T);
  float* d_scores = ctx->d_out.as<float>();
  int* d_best = reinterpret_cast<int*>(d_scores + 2 * N);
  rc = launch_score(ctx, fit.T, m, mode, gate_deg, d_scores, nullptr, d_best, st);
  if (rc != PGP_OK) return rc;
  unsigned char* pin_out = pin + ((in_bytes + 63) & ~(size_t)63);
  PGP_HIP(hipMemcpyAsync(pin_out, d_scores, N * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipMemcpyAsync(pin_out + N * 4, fit.status, N * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipMemcpyAsync(pin_out + N * 8, d_best, 8, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  std::memcpy(scores, pin_out, N * 4);
  std::memcpy(status, pin_out + N * 4, N * 4);
  int best[2];
  std::memcpy(best, pin_out + N * 8, sizeof best);
  if (best_index) *best_index = best[0];
  if (best_score) std::memcpy(best_score, &best[1], 4);
  ctx->csb_fit_m = m;
  return PGP_OK;
}

int pgp_congruent_batch_fetch(pgp_ctx* ctx, const int* index, int k, float* T, double* pose) {
  if (!ctx || k < 0 || (k > 0 && !index)) {
    set_error("pgp_congruent_batch_fetch: bad argument");
    return PGP_EINVAL;
  }
  if (k == 0) return PGP_OK;
  CtxGuard guard(ctx);
  const size_t N = (size_t)ctx->csb_fit_m;
  const RigFits fit = rig_fits(ctx, N);
  if (N == 0 || ctx->d_rig.cap < fit.bytes) {
    set_error("pgp_congruent_batch_fetch: no fits resident (pgp_congruent_batch_fit_score first)");
    return PGP_ESTATE;
  }
  for (int j = 0; j < k; ++j)
    if (index[j] < 0 || (size_t)index[j] >= N) {
      set_error("pgp_congruent_batch_fetch: index %d of %zu", index[j], N);
      return PGP_EINVAL;
    }
  // gathered on the device, ONE copy back through the pinned buffer (a 64-byte copy into pageable memory per
  // entry cost 15 us each: 0.3 ms for the twenty entries of a running-best list)
  const size_t K = (size_t)k, need = K * (4 + 128 + 64) + 256;
  int rc;
  if ((rc = ctx->d_cs_out.ensure(need)) != PGP_OK || (rc = ctx->h_pin.ensure(need)) != PGP_OK) return rc;
  unsigned char* pin = ctx->h_pin.as<unsigned char>();
  unsigned char* dev = ctx->d_cs_out.as<unsigned char>();
  const size_t off_pose = (K * 4 + 127) & ~(size_t)127, off_T = off_pose + K * 128;
  std::memcpy(pin, index, K * 4);
  PGP_HIP(hipMemcpyAsync(dev, pin, K * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(gather_fits, dim3((k + 3) / 4), dim3(64), 0, ctx->stream, reinterpret_cast<const int*>(dev), k,
                     (const float*)fit.T, (const double*)fit.pose, reinterpret_cast<float*>(dev + off_T),
                     reinterpret_cast<double*>(dev + off_pose));
  PGP_HIP(hipMemcpyAsync(pin + off_pose, dev + off_pose, K * (128 + 64), hipMemcpyDeviceToHost, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  if (pose) std::memcpy(pose, pin + off_pose, K * 128);
  if (T) std::memcpy(T, pin + off_T, K * 64);
  return PGP_OK;
}

}  // extern "C"

namespace pgp {
namespace {
// The drop-in's draw of at most `cap` quads per base (base.cc:1858-1866) as a function of (seed, base, quads of the base)
// alone.  Every base has a COUNTER-BASED generator of its own: variate i is splitmix64's finaliser of state + (i + 1) * gamma, the
// state mixed out of the seed and the base's number -- so a wave computes all `cap` variates at once.  The subset is Floyd's: for
// i = 0 .. cap-1, with j = n - cap + i: t = (variate i >> 33) % (j + 1) (31-bit values, as rand() gives); t joins the sample
// unless it is in it already, in which case j does.  Exactly `cap` steps whatever n (drawing until `cap` different values have
// come takes ~5 n draws when n is barely above cap), every subset equally likely; handed out in ascending order; a base with
// fewer than `cap` quads hands out all of them.  The reference draws from the process's rand(), seeded from the clock: any
// uniform sample of `cap` distinct quads is its behaviour.  sample_quads_kernel and pgp_sample_quads: bit for bit the same picks.
// (sample_state / sample_variate: pgp_internal.h, shared with the plane fit's draw)
constexpr int kSampleMax = 128;   // two slots per lane of the base's wave

// one wave per base: where the base's picks start (the sum of the earlier bases' counts), then its draw
__global__ __launch_bounds__(64) void sample_quads_kernel(const uint32_t* __restrict__ base_start, int nb, int cap, unsigned long long seed,
                                                          const int4* __restrict__ base_ids, int2* __restrict__ picks,
                                                          int4* __restrict__ pick_bases) {
  const int b = blockIdx.x, lane = threadIdx.x;
  uint32_t off = 0;
  for (int i = lane; i < b; i += 64) off += min(base_start[i + 1] - base_start[i], (uint32_t)cap);
  off = wave::sum(off);
  const uint32_t nq = base_start[b + 1] - base_start[b];
  const int4 ids = base_ids[b];
  if (nq < (uint32_t)cap) {
    for (uint32_t j = lane; j < nq; j += 64) {
      picks[off + j] = make_int2(b, (int)j);
      pick_bases[off + j] = ids;
    }
    return;
  }
  // this lane's two candidates of Floyd's steps i = lane and i = lane + 64, all lanes at once
  const unsigned long long x = sample_state(seed, b);
  const uint32_t j0 = nq - (uint32_t)cap + (uint32_t)lane, j1 = j0 + 64u;
  const uint32_t t0 = lane < cap ? sample_variate(x, lane) % (j0 + 1u) : 0u;
  const uint32_t t1 = lane + 64 < cap ? sample_variate(x, lane + 64) % (j1 + 1u) : 0u;
  uint32_t s0 = 0xFFFFFFFFu, s1 = 0xFFFFFFFFu;   // slot `lane` and slot `lane + 64` (no quad is number 2^32 - 1)
  for (int i = 0; i < cap; ++i) {
    // (i is the same in every lane: v_readlane, not a cross-lane permute in the middle of the chain)
    const uint32_t t = (uint32_t)(i < 64 ? __builtin_amdgcn_readlane((int)t0, i) : __builtin_amdgcn_readlane((int)t1, i - 64));
    const uint32_t v = __ballot(s0 == t || s1 == t) != 0ull ? nq - (uint32_t)cap + (uint32_t)i : t;
    if (lane == (i & 63)) {
      if (i < 64) s0 = v;
      else s1 = v;
    }
  }
  // ascending: a value's place is the number of smaller ones
  uint32_t r0 = 0, r1 = 0;
  for (int i = 0; i < cap; ++i) {
    const uint32_t u = (uint32_t)(i < 64 ? __builtin_amdgcn_readlane((int)s0, i) : __builtin_amdgcn_readlane((int)s1, i - 64));
    r0 += u < s0 ? 1u : 0u;
    r1 += u < s1 ? 1u : 0u;
  }
  if (lane < cap) {
    picks[off + r0] = make_int2(b, (int)s0);
    pick_bases[off + r0] = ids;
  }
  if (lane + 64 < cap) {
    picks[off + r1] = make_int2(b, (int)s1);
    pick_bases[off + r1] = ids;
  }
}

struct SampleSpec {
  bool on;
  unsigned long long seed;
  int cap;
  int* picks_out;   // nullable: the picks the device drew, [m][2]
  int* m_out;       // nullable
};

int fit_score_list_impl(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                        const float centroid_Q[3], int mode, float gate_deg, int list_cap, int* n_list,
                        int* list_index, float* list_score, float* list_T, double* list_pose, int* n_pushed,
                        int* best_index, float* best_score, float* best_T, double* best_pose, int* registered,
                        int* n_registered, const SampleSpec& smp);
}  // namespace
}  // namespace pgp

extern "C" {

int pgp_sample_quads(unsigned long long seed, const int* n_quads, int n_bases, int max_per_base, int* picks, int* n_picks) {
  if (n_bases < 0 || (n_bases > 0 && !n_quads) || max_per_base < 1 || max_per_base > kSampleMax || !n_picks) {
    set_error("pgp_sample_quads: bad argument (1 <= max_per_base <= %d)", kSampleMax);
    return PGP_EINVAL;
  }
  int k = 0;
  std::vector<unsigned int> got;
  for (int b = 0; b < n_bases; ++b) {
    const int nq = n_quads[b];
    if (nq < 0) {
      set_error("pgp_sample_quads: base %d has %d quads", b, nq);
      return PGP_EINVAL;
    }
    if (nq < max_per_base) {
      for (int j = 0; j < nq; ++j, ++k)
        if (picks) { picks[2 * (size_t)k] = b; picks[2 * (size_t)k + 1] = j; }
      continue;
    }
    got.clear();
    const unsigned long long x = sample_state(seed, b);
    for (int i = 0; i < max_per_base; ++i) {   // Floyd's steps (see sample_quads_kernel)
      const unsigned int j = (unsigned int)(nq - max_per_base + i);
      const unsigned int t = sample_variate(x, i) % (j + 1u);
      got.push_back(std::find(got.begin(), got.end(), t) == got.end() ? t : j);
    }
    std::sort(got.begin(), got.end());
    for (unsigned int v : got) {
      if (picks) { picks[2 * (size_t)k] = b; picks[2 * (size_t)k + 1] = (int)v; }
      ++k;
    }
  }
  *n_picks = k;
  return PGP_OK;
}

int pgp_congruent_batch_fit_score_list(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                                       const float centroid_Q[3], int mode, float gate_deg, int list_cap, int* n_list,
                                       int* list_index, float* list_score, float* list_T, double* list_pose, int* n_pushed,
                                       int* best_index, float* best_score, float* best_T, double* best_pose, int* registered,
                                       int* n_registered) {
  if (m > 0 && !picks) {
    set_error("pgp_congruent_batch_fit_score_list: bad argument");
    return PGP_EINVAL;
  }
  return fit_score_list_impl(ctx, picks, base_ids, m, centroid_P, centroid_Q, mode, gate_deg, list_cap, n_list, list_index, list_score,
                             list_T, list_pose, n_pushed, best_index, best_score, best_T, best_pose, registered, n_registered,
                             SampleSpec{false, 0ull, 0, nullptr, nullptr});
}

int pgp_congruent_batch_sample_fit_score_list(pgp_ctx* ctx, unsigned long long seed, int max_per_base, const int* base_ids,
                                              const float centroid_P[3], const float centroid_Q[3], int mode, float gate_deg,
                                              int list_cap, int* n_list, int* list_index, float* list_score, float* list_T,
                                              double* list_pose, int* n_pushed, int* best_index, float* best_score, float* best_T,
                                              double* best_pose, int* registered, int* n_registered, int* picks_out, int* n_picks) {
  if (max_per_base < 1 || max_per_base > kSampleMax) {
    set_error("pgp_congruent_batch_sample_fit_score_list: 1 <= max_per_base <= %d", kSampleMax);
    return PGP_EINVAL;
  }
  if (n_picks) *n_picks = 0;
  return fit_score_list_impl(ctx, nullptr, base_ids, 0, centroid_P, centroid_Q, mode, gate_deg, list_cap, n_list, list_index,
                             list_score, list_T, list_pose, n_pushed, best_index, best_score, best_T, best_pose, registered,
                             n_registered, SampleSpec{true, seed, max_per_base, picks_out, n_picks});
}

}  // extern "C"

namespace pgp {
namespace {
int fit_score_list_impl(pgp_ctx* ctx, const int* picks, const int* base_ids, int m, const float centroid_P[3],
                        const float centroid_Q[3], int mode, float gate_deg, int list_cap, int* n_list,
                        int* list_index, float* list_score, float* list_T, double* list_pose, int* n_pushed,
                        int* best_index, float* best_score, float* best_T, double* best_pose, int* registered,
                        int* n_registered, const SampleSpec& smp) {
  if (!ctx || m < 0 || !centroid_P || !centroid_Q || list_cap < 0 || list_cap > 4096 || !n_list || !n_registered ||
      ((m > 0 || smp.on) && !base_ids) || (list_cap > 0 && (!list_index || !list_score || !list_T || !list_pose))) {
    set_error("pgp_congruent_batch_fit_score_list: bad argument");
    return PGP_EINVAL;
  }
  if (smp.on) {
    // the picks are drawn on the device; how many there will be follows from the resident batch's quad counts
    if (ctx->csb_nb <= 0 || (int)ctx->csb_starts.size() != ctx->csb_nb + 1) {
      set_error("pgp_congruent_batch_sample_fit_score_list: no congruent batch resident (pgp_find_congruent_batch first)");
      return PGP_ESTATE;
    }
    long long total = 0;
    for (int b = 0; b < ctx->csb_nb; ++b)
      total += std::min<long long>((long long)(ctx->csb_starts[b + 1] - ctx->csb_starts[b]), smp.cap);
    if (total > 0x3FFFFFFF) {
      set_error("pgp_congruent_batch_sample_fit_score_list: more than 2^30 picks");
      return PGP_EINVAL;
    }
    m = (int)total;
    if (smp.m_out) *smp.m_out = m;
  }
  *n_list = 0;
  *n_registered = 0;
  if (n_pushed) *n_pushed = 0;
  if (best_index) *best_index = -1;
  if (best_score) *best_score = 0.f;
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)m, C = (size_t)list_cap, nQ = (size_t)std::max(ctx->nQ, 0);
  int rc;
  if ((rc = pgp_reserve(ctx, m)) != PGP_OK) return rc;
  if ((rc = ctx->d_ids.ensure(N * 40 + 64 + (size_t)std::max(ctx->csb_nb, 0) * 16 + 64)) != PGP_OK) return rc;   // bases of the picks | picks | quads | ids of the bases
  ctx->csb_fit_m = 0;
  if ((rc = ctx->d_rig.ensure(rig_fits(ctx, N).bytes)) != PGP_OK) return rc;
  // scores | (counts) | best -- then what goes home in ONE copy: best {index, score bits} | list {records, pushed, indices}
  // | record scores | poses (records, best) | transforms (records, best) | hits of the best pose
  const size_t off_best = N * 8, off_list = off_best + 16, off_rs = off_list + (C + 2) * 4, off_pose = (off_rs + C * 4 + 127) & ~(size_t)127,
               off_T = off_pose + (C + 1) * 128, off_hits = off_T + (C + 1) * 64, total = off_hits + nQ * 4 + 64;
  if ((rc = ctx->d_out.ensure(total)) != PGP_OK) return rc;
  const size_t in_bytes = smp.on ? (((size_t)std::max(ctx->csb_nb, 0) * 16 + 63) & ~(size_t)63) : N * 24;   // bases of the picks | picks
  const size_t home = total - off_best, pin_need = in_bytes + home + (smp.on && smp.picks_out ? N * 8 + 64 : 0) + 256;
  if ((rc = ctx->h_pin.ensure(pin_need)) != PGP_OK) return rc;
  unsigned char* pin = ctx->h_pin.as<unsigned char>();
  int* hb = reinterpret_cast<int*>(pin);
  // device: bases of the picks [4 N] | picks [2 N] (ONE copy) | quads [4 N] | (sampled form) the bases' ids [4 nb]
  int* d_b = ctx->d_ids.as<int>();
  int* d_pk = d_b + 4 * N;
  int* d_q = d_pk + ((2 * N + 3) & ~(size_t)3);   // (int4 records: 16-byte aligned)
  if (!smp.on) {
    if (!pick_bases(picks, N, base_ids, hb, ctx->csb_nb, "pgp_congruent_batch_fit_score_list")) return PGP_EINVAL;
    std::memcpy(hb + 4 * N, picks, N * 8);
    if ((rc = stage_to_device(st, d_b, hb, in_bytes)) != PGP_OK) return rc;
    rc = launch_congruent_batch_gather(ctx, picks, m, reinterpret_cast<int4*>(d_q), st, reinterpret_cast<const int2*>(d_pk));
    if (rc != PGP_OK) return rc;
  } else {
    // the bases' ids go up (16 B each), the picks are drawn where the quads are: one wave per base
    const int nb = ctx->csb_nb;
    int* d_base_ids = d_q + 4 * N;
    std::memcpy(hb, base_ids, (size_t)nb * 16);
    if ((rc = stage_to_device(st, d_base_ids, hb, (size_t)nb * 16)) != PGP_OK) return rc;
    const uint32_t* d_base_start = congruent_batch_starts_device(ctx);
    hipLaunchKernelGGL(sample_quads_kernel, dim3((unsigned)nb), dim3(64), 0, st, d_base_start, nb, smp.cap, smp.seed,
                       reinterpret_cast<const int4*>(d_base_ids), reinterpret_cast<int2*>(d_pk), reinterpret_cast<int4*>(d_b));
    PGP_HIP(hipGetLastError());
    rc = launch_congruent_batch_gather(ctx, nullptr, m, reinterpret_cast<int4*>(d_q), st, reinterpret_cast<const int2*>(d_pk));
    if (rc != PGP_OK) return rc;
  }
  const RigFits fit = rig_fits(ctx, N);
  rc = launch_rigid(ctx, d_b, d_q, m, centroid_P, centroid_Q, fit.T, fit.pose, fit.status, fit.rms, st);
  if (rc != PGP_OK) return rc;
  hipLaunchKernelGGL(mask_failed_fits, dim3((m + 255) / 256), dim3(256), 0, st, (const int*)fit.status, m, fit.T);
  unsigned char* dev = ctx->d_out.as<unsigned char>();
  float* d_scores = reinterpret_cast<float*>(dev);
  int* d_best = reinterpret_cast<int*>(dev + off_best);
  int* d_list = reinterpret_cast<int*>(dev + off_list);
  float* d_rs = reinterpret_cast<float*>(dev + off_rs);
  double* d_pose_out = reinterpret_cast<double*>(dev + off_pose);
  float* d_T_out = reinterpret_cast<float*>(dev + off_T);
  int* d_hits = reinterpret_cast<int*>(dev + off_hits);
  rc = launch_score(ctx, fit.T, m, mode, gate_deg, d_scores, nullptr, d_best, st);
  if (rc != PGP_OK) return rc;
  // the walk, the poses it keeps, the best pose and the points it registers: all behind the scores on the stream
  hipLaunchKernelGGL(records_walk, dim3(1), dim3(256), 0, st, m, (const float*)d_scores, (const int*)fit.status, list_cap, d_list, d_rs);
  hipLaunchKernelGGL(gather_fits_list, dim3((list_cap + 1 + 3) / 4), dim3(64), 0, st, (const int*)d_list, list_cap, (const int*)d_best,
                     (const float*)fit.T, (const double*)fit.pose, d_T_out, d_pose_out);
  PGP_HIP(hipGetLastError());
  if (nQ > 0 && (rc = launch_registered(ctx, d_T_out + 16 * C, mode, gate_deg, d_hits, st)) != PGP_OK) return rc;
  unsigned char* pin_out = pin + ((in_bytes + 63) & ~(size_t)63);
  {
    // one kernel brings everything home and writes the word the host polls (pgp::publish_and_wait); the build that was put
    // off goes to its stream first, as before any wait of the host
    if (ctx->deferred_build && (rc = flush_deferred_build(ctx)) != PGP_OK) return rc;
    unsigned char* pin_picks = pin_out + ((home + 63) & ~(size_t)63);
    const bool want_picks = smp.on && smp.picks_out;
    const PubItem items[2] = {{dev + off_best, pin_out, home}, {d_pk, pin_picks, N * 8}};
    const int n_items = want_picks ? 2 : 1;
    if (publish_usable(items, n_items)) {
      if ((rc = publish_and_wait(ctx, st, items, n_items)) != PGP_OK) return rc;
    } else {
      PGP_HIP(hipMemcpyAsync(pin_out, dev + off_best, home, hipMemcpyDeviceToHost, st));
      if (want_picks) PGP_HIP(hipMemcpyAsync(pin_picks, d_pk, N * 8, hipMemcpyDeviceToHost, st));
      PGP_HIP(hipStreamSynchronize(st));
    }
    if (want_picks) std::memcpy(smp.picks_out, pin_picks, N * 8);
  }
  if ((rc = index_settled(ctx)) != PGP_OK) return rc;
  const unsigned char* h = pin_out - off_best;   // (offsets as on the device)
  int best[2], lst[2];
  std::memcpy(best, h + off_best, sizeof best);
  std::memcpy(lst, h + off_list, sizeof lst);
  *n_list = lst[0];
  if (n_pushed) *n_pushed = lst[1];
  if (best_index) *best_index = best[0];
  if (best_score) std::memcpy(best_score, &best[1], 4);
  const size_t n_rec = (size_t)std::min(std::max(lst[0], 0), list_cap);
  if (n_rec) {
    std::memcpy(list_index, h + off_list + 8, n_rec * 4);
    std::memcpy(list_score, h + off_rs, n_rec * 4);
    std::memcpy(list_pose, h + off_pose, n_rec * 128);
    std::memcpy(list_T, h + off_T, n_rec * 64);
  }
  if (best[0] >= 0) {
    if (best_pose) std::memcpy(best_pose, h + off_pose + C * 128, 128);
    if (best_T) std::memcpy(best_T, h + off_T + C * 64, 64);
    if (registered) {
      const int* hits = reinterpret_cast<const int*>(h + off_hits);
      int k = 0;
      for (size_t i = 0; i < nQ; ++i)
        if (hits[i] >= 0) registered[k++] = hits[i];   // model-point order, as push_back in base.cc:1760
      *n_registered = k;
    }
  }
  ctx->csb_fit_m = m;
  return PGP_OK;
}
}  // namespace
}  // namespace pgp

extern "C" {

static pgp_icp_options options_of(const pgp_icp_params* p) {
  pgp_icp_options o;
  pgp_icp_default_options(&o);
  o.max_iterations = p->max_iterations;
  o.trim_fraction = p->trim_fraction;
  o.max_corr_dist = p->max_corr_dist;
  o.energy_ratio = p->energy_ratio > 0.f ? p->energy_ratio : 1.f;   // setNewToOldEnergyRatio(1.f), UCTState.cpp:139
  return o;
}

int pgp_icp_default_options(pgp_icp_options* opt) {
  if (!opt) {
    set_error("pgp_icp_default_options: opt is NULL");
    return PGP_EINVAL;
  }
  opt->max_iterations = 100;
  opt->trim_fraction = 1.f;
  opt->max_corr_dist = 0.f;
  opt->energy_ratio = 1.f;
  opt->error_metric = 0;
  opt->transformation_epsilon = -1.f;
  opt->relative_mse = 0.f;
  opt->absolute_mse = -1.f;
  opt->min_diff_rot = 0.f;
  opt->min_diff_trans = 0.f;
  opt->smooth_length = 0;
  opt->nn_search = 0;
  return PGP_OK;
}

int pgp_icp_refine_ex_device(pgp_ctx* ctx, const float* d_src4, int n_src, const float* d_tgt4,
                             const float* d_tgt_n4, int n_tgt, float* d_T, int n, const pgp_icp_options* opt,
                             float* d_energy, int* d_iters, void* stream) {
  if (!ctx || !opt || n < 0 || n_src < 0 || n_tgt < 0 || (n > 0 && (!d_src4 || !d_tgt4 || !d_T))) {
    set_error("pgp_icp_refine_ex_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  const int rc = launch_icp(ctx, reinterpret_cast<const float4*>(d_src4), n_src, reinterpret_cast<const float4*>(d_tgt4),
                    reinterpret_cast<const float4*>(d_tgt_n4), n_tgt, d_T, n, opt, d_energy, d_iters,
                    static_cast<hipStream_t>(stream), ctx->icp_user_token);
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_select_top_device(pgp_ctx* ctx, const float* d_T, const float* d_scores, int n, int k, int invert,
                          float* d_T_out, int* d_index_out, int* d_n_out, void* stream) {
  if (!ctx || n < 0 || k < 0 || (k > 0 && (!d_T_out || !d_n_out)) || (n > 0 && (!d_T || !d_scores))) {
    set_error("pgp_select_top_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  const int rc = launch_select_top(ctx, d_T, d_scores, n, k, invert, d_T_out, d_index_out, d_n_out, static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_icp_refine_multi_device(const pgp_icp_job* jobs, int n_jobs, const pgp_icp_params* params, void* stream) {
  if (n_jobs < 0 || (n_jobs > 0 && !jobs) || !params) {
    set_error("pgp_icp_refine_multi_device: bad argument");
    return PGP_EINVAL;
  }
  if (n_jobs == 0) return PGP_OK;
  std::vector<IcpJob> v((size_t)n_jobs);
  for (int j = 0; j < n_jobs; ++j) {
    const pgp_icp_job& q = jobs[j];
    if (!q.ctx || q.n < 0 || q.n_src < 0 || q.n_tgt < 0 || (q.n > 0 && (!q.d_src4 || !q.d_tgt4 || !q.d_T))) {
      set_error("pgp_icp_refine_multi_device: bad job %d", j);
      return PGP_EINVAL;
    }
    v[j] = IcpJob{q.ctx, reinterpret_cast<const float4*>(q.d_src4), q.n_src, reinterpret_cast<const float4*>(q.d_tgt4), q.n_tgt,
                  q.d_T, q.n, q.d_energy, q.d_iters, q.ctx->icp_user_token};
  }
  const pgp_icp_options o = options_of(params);
  CtxGuard guard(jobs[0].ctx, false);
  const int rc = launch_icp_multi(v.data(), n_jobs, &o, static_cast<hipStream_t>(stream));
  for (int j = 0; j < n_jobs; ++j) note_device_work(jobs[j].ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_icp_target_token(pgp_ctx* ctx, unsigned long long token) {
  if (!ctx) {
    set_error("pgp_icp_target_token: ctx is NULL");
    return PGP_EINVAL;
  }
  ctx->icp_user_token = token;
  return PGP_OK;
}

int pgp_icp_refine_device(pgp_ctx* ctx, const float* d_src4, int n_src, const float* d_tgt4, int n_tgt,
                          float* d_T, int n, const pgp_icp_params* params, float* d_energy,
                          int* d_iters, void* stream) {
  if (!params) {
    set_error("pgp_icp_refine_device: bad argument");
    return PGP_EINVAL;
  }
  const pgp_icp_options o = options_of(params);
  return pgp_icp_refine_ex_device(ctx, d_src4, n_src, d_tgt4, nullptr, n_tgt, d_T, n, &o, d_energy, d_iters, stream);
}

}  // extern "C"

namespace pgp {

pgp_icp_options icp_options_of(const pgp_icp_params* p) { return options_of(p); }

namespace {
std::vector<float4> pack4(const float* xyz, int m) {
  std::vector<float4> v((size_t)std::max(m, 1));
  for (int i = 0; i < m; ++i) v[i] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.f);
  return v;
}
// The target is the object's model, the same from call to call (TrimmedICP::init builds its search
// structure once per model: UCTState.cpp:137-139): a hash of its coordinates tells whether the copy
// and the index already resident on the device are this target's, and the upload + build are skipped.
unsigned long long hash_of(const float* xyz, int m) {
  // eight independent multiply-xor chains over the 64-bit words (a single chain over 32-bit words is latency-bound: 20 us
  // at 5000 points; four of them still took ~0.1 ms on the 100 000-point table of the scene alignment, SceneCfg.cpp:135-141)
  const size_t e32 = 3 * (size_t)m, e = e32 / 2;
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(xyz);
  unsigned long long h[8] = {0x9E3779B97F4A7C15ull ^ (unsigned long long)m, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull,
                             0x85EBCA77C2B2AE63ull, 0xD6E8FEB86659FD93ull, 0xFF51AFD7ED558CCDull, 0xC4CEB9FE1A85EC53ull};
  size_t i = 0;
  for (; i + 8 <= e; i += 8) {
    unsigned long long w[8];
    std::memcpy(w, bytes + 8 * i, 64);
#pragma GCC unroll 8
    for (int k = 0; k < 8; ++k) h[k] = (h[k] ^ w[k]) * 0x100000001B3ull + (h[k] >> (27 + k % 5));
  }
  for (; i < e; ++i) {
    unsigned long long w;
    std::memcpy(&w, bytes + 8 * i, 8);
    h[0] = (h[0] ^ w) * 0x100000001B3ull + (h[0] >> 29);
  }
  if (e32 & 1) {
    uint32_t w;
    std::memcpy(&w, bytes + 4 * (e32 - 1), 4);
    h[1] = (h[1] ^ w) * 0x100000001B3ull + (h[1] >> 31);
  }
  unsigned long long hsh = h[0];
  for (int k = 1; k < 8; ++k) hsh = (hsh ^ (h[k] << (7 * k) | h[k] >> (64 - 7 * k))) * 0x9E3779B97F4A7C15ull;
  return hsh | 1ull;   // never 0
}
}  // namespace

// One host-pointer ICP job staged in the context's buffers on `st` (no launch yet): ONE device block
// [src | T | energy | iters] and its pinned host image -- ONE copy in ([src | T]) and ONE copy out
// ([T | energy | iters]): the caller's arrays are pageable, and five pageable copies cost more than ten
// ICP iterations of one pose.  The target goes to d_icp_tgt unless its hash says it is resident.
int icp_host_stage(pgp_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt, const float* T, int n,
                   hipStream_t st, IcpHostStage* out) {
  int rc;
  IcpHostStage g{};
  g.off_T = (size_t)std::max(n_src, 1) * 16;
  g.off_e = g.off_T + (size_t)n * 64;
  g.off_i = g.off_e + (size_t)n * 4;
  g.total = g.off_i + (size_t)n * 4;
  if ((rc = ctx->d_icp_src.ensure(g.total)) != PGP_OK) return rc;
  if ((rc = ctx->d_icp_tgt.ensure((size_t)std::max(n_tgt, 1) * 16)) != PGP_OK) return rc;
  if ((rc = ctx->h_pin.ensure(g.total + 64)) != PGP_OK) return rc;
  unsigned char* pin = ctx->h_pin.as<unsigned char>();
  {
    float4* ps = reinterpret_cast<float4*>(pin);
    for (int i = 0; i < n_src; ++i)
      ps[i] = make_float4(src_xyz[3 * (size_t)i], src_xyz[3 * (size_t)i + 1], src_xyz[3 * (size_t)i + 2], 0.f);
    std::memcpy(pin + g.off_T, T, (size_t)n * 64);
  }
  const unsigned long long tok = hash_of(tgt_xyz, n_tgt);
  if (!(tok == ctx->icp_host_token && n_tgt == ctx->icp_host_ntgt)) {
    const std::vector<float4> ht = pack4(tgt_xyz, n_tgt);
    ctx->icp_host_token = 0;
    ctx->icp_idx_valid = false;
    ctx->icp_grid_valid = false;
    PGP_HIP(hipMemcpyAsync(ctx->d_icp_tgt.p, ht.data(), (size_t)n_tgt * 16, hipMemcpyHostToDevice, st));
    PGP_HIP(hipStreamSynchronize(st));   // ht is a temporary
    ctx->icp_host_token = tok;
    ctx->icp_host_ntgt = n_tgt;
  }
  unsigned char* dev = ctx->d_icp_src.as<unsigned char>();
  g.d_src = reinterpret_cast<const float4*>(dev);
  g.d_tgt = ctx->d_icp_tgt.as<float4>();
  g.d_T = reinterpret_cast<float*>(dev + g.off_T);
  g.d_energy = reinterpret_cast<float*>(dev + g.off_e);
  g.d_iters = reinterpret_cast<int*>(dev + g.off_i);
  g.token = tok;
  if ((rc = stage_to_device(st, dev, pin, g.off_e)) != PGP_OK) return rc;
  *out = g;
  return PGP_OK;
}

// the results' way back: queued behind the job's kernels on `st` ...
int icp_host_collect_enqueue(pgp_ctx* ctx, const IcpHostStage& g, hipStream_t st) {
  unsigned char* pin = ctx->h_pin.as<unsigned char>();
  unsigned char* dev = ctx->d_icp_src.as<unsigned char>();
  PGP_HIP(hipMemcpyAsync(pin + g.off_T, dev + g.off_T, g.total - g.off_T, hipMemcpyDeviceToHost, st));
  return PGP_OK;
}
// ... and, once `st` is synchronised, out of the pinned image into the caller's arrays
void icp_host_collect(pgp_ctx* ctx, const IcpHostStage& g, int n, float* T, float* energy, int* iters) {
  const unsigned char* pin = ctx->h_pin.as<const unsigned char>();
  std::memcpy(T, pin + g.off_T, (size_t)n * 64);
  if (energy) std::memcpy(energy, pin + g.off_e, (size_t)n * 4);
  if (iters) std::memcpy(iters, pin + g.off_i, (size_t)n * 4);
}

}  // namespace pgp

extern "C" {

int pgp_icp_refine_ex(pgp_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, const float* tgt_nrm,
                      int n_tgt, float* T, int n, const pgp_icp_options* opt, float* energy, int* iters) {
  if (!ctx || !opt || n < 0 || n_src < 0 || n_tgt < 0 ||
      (n > 0 && (!T || (n_src > 0 && !src_xyz) || (n_tgt > 0 && !tgt_xyz)))) {
    set_error("pgp_icp_refine_ex: bad argument");
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  int rc;
  IcpHostStage g{};
  if ((rc = icp_host_stage(ctx, src_xyz, n_src, tgt_xyz, n_tgt, T, n, st, &g)) != PGP_OK) return rc;
  const float4* d_n = nullptr;
  if (tgt_nrm) {
    const unsigned long long ntok = hash_of(tgt_nrm, n_tgt);
    if ((rc = ctx->d_icp_tgt_n.ensure((size_t)std::max(n_tgt, 1) * 16)) != PGP_OK) return rc;
    if (ntok != ctx->icp_host_ntoken) {
      const std::vector<float4> hn = pack4(tgt_nrm, n_tgt);
      ctx->icp_host_ntoken = 0;
      PGP_HIP(hipMemcpyAsync(ctx->d_icp_tgt_n.p, hn.data(), (size_t)n_tgt * 16, hipMemcpyHostToDevice, st));
      PGP_HIP(hipStreamSynchronize(st));
      ctx->icp_host_ntoken = ntok;
    }
    d_n = ctx->d_icp_tgt_n.as<float4>();
  }
  rc = launch_icp(ctx, g.d_src, n_src, g.d_tgt, d_n, n_tgt, g.d_T, n, opt, g.d_energy, g.d_iters, st, g.token);
  if (rc != PGP_OK) return rc;
  // the results' way home: one publishing kernel + the completion word (pgp::publish_and_wait) where they are small and aligned,
  // else a copy and the stream
  auto home = [&]() -> int {
    const PubItem item{ctx->d_icp_src.as<unsigned char>() + g.off_T, ctx->h_pin.as<unsigned char>() + g.off_T, g.total - g.off_T};
    if (publish_usable(&item, 1)) return publish_and_wait(ctx, st, &item, 1);
    const int r = icp_host_collect_enqueue(ctx, g, st);
    if (r != PGP_OK) return r;
    PGP_HIP(hipStreamSynchronize(st));
    return PGP_OK;
  };
  if ((rc = home()) != PGP_OK) return rc;
  {
    // A pose the scene-sized one-launch form gave up on (iteration count -1: the device was held by somebody else for
    // seconds and the pose's units did not arrive, icp.hip icp_scene_persist) -- the caller's transforms are still
    // untouched: the whole job once more, host-driven.
    const int* it = reinterpret_cast<const int*>(ctx->h_pin.as<const unsigned char>() + g.off_i);
    bool lost = false;
    for (int i = 0; i < n; ++i) lost = lost || it[i] < 0;
    if (lost) {
      if ((rc = icp_host_stage(ctx, src_xyz, n_src, tgt_xyz, n_tgt, T, n, st, &g)) != PGP_OK) return rc;
      rc = launch_icp(ctx, g.d_src, n_src, g.d_tgt, d_n, n_tgt, g.d_T, n, opt, g.d_energy, g.d_iters, st, g.token, true);
      if (rc != PGP_OK) return rc;
      if ((rc = home()) != PGP_OK) return rc;
    }
  }
  icp_host_collect(ctx, g, n, T, energy, iters);
  return PGP_OK;
}

int pgp_icp_refine(pgp_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt,
                   float* T, int n, const pgp_icp_params* params, float* energy, int* iters) {
  if (!params) {
    set_error("pgp_icp_refine: bad argument");
    return PGP_EINVAL;
  }
  const pgp_icp_options o = options_of(params);
  return pgp_icp_refine_ex(ctx, src_xyz, n_src, tgt_xyz, nullptr, n_tgt, T, n, &o, energy, iters);
}

int pgp_radius_outlier_filter(pgp_ctx* ctx, const float* xyz, const float* nrm, int n, float radius,
                              int min_neighbors, unsigned char* keep, float* nrm_out, int* n_kept) {
  if (!ctx || n < 0 || (n > 0 && (!xyz || !keep)) || !(radius > 0.f) || !n_kept) {
    set_error("pgp_radius_outlier_filter: bad argument");
    return PGP_EINVAL;
  }
  *n_kept = 0;
  if (n == 0) return PGP_OK;
  // the scene index with delta = radius answers "points within radius" for the cloud itself
  int rc = pgp_set_scene(ctx, xyz, nullptr, nullptr, n, radius);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx);
  if ((rc = ctx->d_counts.ensure((size_t)n * sizeof(int))) != PGP_OK) return rc;
  rc = launch_count_neighbours(ctx, radius, ctx->d_counts.as<int>(), ctx->stream);
  if (rc != PGP_OK) return rc;
  std::vector<int> k((size_t)n);
  PGP_HIP(hipMemcpyAsync(k.data(), ctx->d_counts.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    keep[i] = k[i] > min_neighbors ? 1 : 0;  // PCL 1.7: `k <= min_pts_radius_` -> outlier
    kept += keep[i];
    if (nrm && nrm_out) {
      // pcl::flipNormalTowardsViewpoint(p, 0,0,0, n): flip when (vp - p).n < 0, then / magnitude
      const float* p = xyz + 3 * (size_t)i;
      float nx = nrm[3 * (size_t)i], ny = nrm[3 * (size_t)i + 1], nz = nrm[3 * (size_t)i + 2];
      const float vx = 0.f - p[0], vy = 0.f - p[1], vz = 0.f - p[2];
      const float cos_theta = vx * nx + vy * ny + vz * nz;
      if (cos_theta < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
      const float mag = std::sqrt(nx * nx + ny * ny + nz * nz);
      nrm_out[3 * (size_t)i] = nx / mag;
      nrm_out[3 * (size_t)i + 1] = ny / mag;
      nrm_out[3 * (size_t)i + 2] = nz / mag;
    }
  }
  *n_kept = kept;
  return PGP_OK;
}

int pgp_unexplained_segment(pgp_ctx* ctx, const float* seg_xyz, int n, const float* model_xyz, const int* model_offsets,
                            const float* T, int n_objects, float radius, unsigned char* keep, int* n_kept) {
  if (!ctx || n < 0 || n_objects < 0 || (n > 0 && (!seg_xyz || !keep)) || !(radius > 0.f) ||
      (n_objects > 0 && (!model_offsets || !T))) {
    set_error("pgp_unexplained_segment: bad argument");
    return PGP_EINVAL;
  }
  if (n_kept) *n_kept = 0;
  if (n == 0) return PGP_OK;
  int n_model = 0;
  for (int k = 0; k < n_objects; ++k) {
    if (model_offsets[k] < 0 || model_offsets[k + 1] < model_offsets[k]) {
      set_error("pgp_unexplained_segment: model_offsets must be non-decreasing from 0");
      return PGP_EINVAL;
    }
    n_model = model_offsets[k + 1];
  }
  if (n_model > 0 && !model_xyz) {
    set_error("pgp_unexplained_segment: model_xyz is NULL");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t off_m = up((size_t)n * 12), off_o = off_m + up((size_t)std::max(n_model, 1) * 12),
               off_T = off_o + up(((size_t)n_objects + 1) * 4), off_e = off_T + up((size_t)std::max(n_objects, 1) * 64),
               total = off_e + (size_t)n * 4;
  int rc = ctx->d_pre_io.ensure(total);
  if (rc != PGP_OK) return rc;
  unsigned char* d = ctx->d_pre_io.as<unsigned char>();
  PGP_HIP(hipMemcpyAsync(d, seg_xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
  if (n_objects > 0) {
    if (n_model > 0) PGP_HIP(hipMemcpyAsync(d + off_m, model_xyz, (size_t)n_model * 12, hipMemcpyHostToDevice, st));
    PGP_HIP(hipMemcpyAsync(d + off_o, model_offsets, ((size_t)n_objects + 1) * 4, hipMemcpyHostToDevice, st));
    PGP_HIP(hipMemcpyAsync(d + off_T, T, (size_t)n_objects * 64, hipMemcpyHostToDevice, st));
  }
  rc = launch_explained_points(ctx, reinterpret_cast<const float*>(d), n, reinterpret_cast<const float*>(d + off_m),
                               reinterpret_cast<const int*>(d + off_o), reinterpret_cast<const float*>(d + off_T), n_objects,
                               radius, reinterpret_cast<unsigned int*>(d + off_e), st);
  if (rc != PGP_OK) return rc;
  std::vector<unsigned int> he((size_t)n);
  PGP_HIP(hipMemcpyAsync(he.data(), d + off_e, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    keep[i] = he[i] ? 0 : 1;
    kept += keep[i];
  }
  if (n_kept) *n_kept = kept;
  return PGP_OK;
}

int pgp_backproject_depth(pgp_ctx* ctx, const void* image, int raw16, const unsigned char* mask, int rows,
                          int cols, const float K[9], double z_min, double z_max, float* xyz_out, int cap,
                          int* n_out) {
  if (!ctx || rows < 0 || cols < 0 || cap < 0 || !K || !n_out || (cap > 0 && !xyz_out) ||
      ((size_t)rows * cols > 0 && !image) || (size_t)rows * cols > ((size_t)1 << 30)) {
    set_error("pgp_backproject_depth: bad argument");
    return PGP_EINVAL;
  }
  *n_out = 0;
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t img_bytes = (n * (raw16 ? 2 : 4) + 255) & ~(size_t)255;
  const size_t mask_bytes = (n + 255) & ~(size_t)255;
  const size_t nb = (n + 255) / 256;
  const size_t ctr_bytes = ((nb + 1) * 4 + 255) & ~(size_t)255;
  const size_t scan_bytes = ((nb / 2048 + 4) * 4 + 255) & ~(size_t)255;
  const size_t xyz_bytes = (size_t)cap * 12;
  int rc = ctx->d_bp.ensure(img_bytes + mask_bytes + ctr_bytes + scan_bytes + xyz_bytes + 256);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_bp.as<unsigned char>();
  void* d_img = base;
  unsigned char* d_mask = mask ? base + img_bytes : nullptr;
  uint32_t* d_ctr = reinterpret_cast<uint32_t*>(base + img_bytes + mask_bytes);
  uint32_t* d_scan = reinterpret_cast<uint32_t*>(base + img_bytes + mask_bytes + ctr_bytes);
  float* d_xyz = reinterpret_cast<float*>(base + img_bytes + mask_bytes + ctr_bytes + scan_bytes);
  PGP_HIP(hipMemcpyAsync(d_img, image, n * (raw16 ? 2 : 4), hipMemcpyHostToDevice, st));
  if (mask) PGP_HIP(hipMemcpyAsync(d_mask, mask, n, hipMemcpyHostToDevice, st));
  int total = 0;
  rc = launch_backproject(ctx, d_img, raw16 != 0, d_mask, rows, cols, K, z_min, z_max, d_ctr, d_scan, d_xyz, cap,
                          &total, st);
  if (rc != PGP_OK) return rc;
  *n_out = total;
  const int n_copy = total < cap ? total : cap;
  if (n_copy > 0) {
    HostOut out(ctx, st);
    if ((rc = out.to(xyz_out, d_xyz, (size_t)n_copy * 12)) != PGP_OK || (rc = out.sync()) != PGP_OK) return rc;
  }
  return PGP_OK;
}

int pgp_set_scene_device(pgp_ctx* ctx, const float* d_xyz, const float* d_nrm, const float* d_weight, int n,
                         float delta, void* stream) {
  if (!ctx || n < 0 || (n > 0 && !d_xyz) || !(delta > 0.f) || !std::isfinite(delta)) {
    set_error("pgp_set_scene_device: bad argument (n=%d, delta=%g)", n, (double)delta);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PGP_HIP(hipStreamSynchronize(st));   // the producer of d_xyz
  PGP_HIP(hipDeviceSynchronize());     // queued launches may still read the arrays replaced below
  return set_scene_device(ctx, d_xyz, d_nrm, d_weight, n, delta, st);
}

int pgp_voxel_grid_device(pgp_ctx* ctx, const float* d_xyz, int n, float leaf, float* d_out_xyz, int cap,
                          int* n_out, void* stream) {
  if (!ctx || n < 0 || cap < 0 || !n_out || !(leaf > 0.f) || !std::isfinite(leaf) || (n > 0 && !d_xyz) ||
      (cap > 0 && !d_out_xyz)) {
    set_error("pgp_voxel_grid_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  return launch_voxel_grid(ctx, d_xyz, n, leaf, d_out_xyz, cap, n_out, static_cast<hipStream_t>(stream));
}

int pgp_voxel_grid(pgp_ctx* ctx, const float* xyz, int n, float leaf, float* out_xyz, int cap, int* n_out) {
  if (!ctx || n < 0 || cap < 0 || !n_out || !(leaf > 0.f) || !std::isfinite(leaf) || (n > 0 && !xyz) ||
      (cap > 0 && !out_xyz)) {
    set_error("pgp_voxel_grid: bad argument");
    return PGP_EINVAL;
  }
  *n_out = 0;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t in_b = ((size_t)n * 12 + 255) & ~(size_t)255;
  int rc = ctx->d_pre_io.ensure(in_b + (size_t)std::max(cap, 1) * 12 + 64);
  if (rc != PGP_OK) return rc;
  float* d_in = ctx->d_pre_io.as<float>();
  float* d_out = reinterpret_cast<float*>(ctx->d_pre_io.as<unsigned char>() + in_b);
  PGP_HIP(hipMemcpyAsync(d_in, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
  rc = launch_voxel_grid(ctx, d_in, n, leaf, d_out, cap, n_out, st);
  if (rc != PGP_OK) return rc;
  const int n_copy = *n_out < cap ? *n_out : cap;
  if (n_copy > 0) {
    HostOut out(ctx, st);
    if ((rc = out.to(out_xyz, d_out, (size_t)n_copy * 12)) != PGP_OK || (rc = out.sync()) != PGP_OK) return rc;
  }
  return PGP_OK;
}

int pgp_mls_normals_device(pgp_ctx* ctx, const float* d_xyz, int n, float radius, float* d_out_xyz, float* d_out_nrm,
                           float* d_out_curvature, int* d_out_index, int cap, int* n_out, void* stream) {
  if (!ctx || n < 0 || cap < 0 || !n_out || !(radius > 0.f) || !std::isfinite(radius) || (n > 0 && !d_xyz) ||
      (cap > 0 && !d_out_xyz)) {
    set_error("pgp_mls_normals_device: bad argument");
    return PGP_EINVAL;
  }
  *n_out = 0;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx, false);
  return launch_mls(ctx, d_xyz, n, radius, d_out_xyz, d_out_nrm, d_out_curvature, d_out_index, cap, n_out,
                    static_cast<hipStream_t>(stream));
}

int pgp_mls_normals(pgp_ctx* ctx, const float* xyz, int n, float radius, float* out_xyz, float* out_nrm,
                    float* out_curvature, int* out_index, int cap, int* n_out) {
  if (!ctx || n < 0 || cap < 0 || !n_out || !(radius > 0.f) || !std::isfinite(radius) || (n > 0 && !xyz) ||
      (cap > 0 && !out_xyz)) {
    set_error("pgp_mls_normals: bad argument");
    return PGP_EINVAL;
  }
  *n_out = 0;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)std::max(cap, 1);
  const size_t b_in = ((size_t)n * 12 + 255) & ~(size_t)255, b_3 = (rows * 12 + 255) & ~(size_t)255,
               b_1 = (rows * 4 + 255) & ~(size_t)255;
  int rc = ctx->d_pre_io.ensure(b_in + 2 * b_3 + 2 * b_1);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_pre_io.as<unsigned char>();
  float* d_in = reinterpret_cast<float*>(base);
  float* d_x = reinterpret_cast<float*>(base + b_in);
  float* d_n = reinterpret_cast<float*>(base + b_in + b_3);
  float* d_c = reinterpret_cast<float*>(base + b_in + 2 * b_3);
  int* d_i = reinterpret_cast<int*>(base + b_in + 2 * b_3 + b_1);
  PGP_HIP(hipMemcpyAsync(d_in, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
  rc = launch_mls(ctx, d_in, n, radius, d_x, d_n, d_c, d_i, cap, n_out, st);
  if (rc != PGP_OK) return rc;
  const size_t m = (size_t)(*n_out < cap ? *n_out : cap);
  if (m > 0) {
    // through the context's pinned landing area, one wait for all four (a copy into the caller's pageable array is a
    // synchronisation of its own: four of them were 160 us of a 0.52 ms call, tools/call_timeline.sh mls)
    HostOut out(ctx, st);
    if ((rc = out.to(out_xyz, d_x, m * 12)) != PGP_OK) return rc;
    if (out_nrm && (rc = out.to(out_nrm, d_n, m * 12)) != PGP_OK) return rc;
    if (out_curvature && (rc = out.to(out_curvature, d_c, m * 4)) != PGP_OK) return rc;
    if (out_index && (rc = out.to(out_index, d_i, m * 4)) != PGP_OK) return rc;
    if ((rc = out.sync()) != PGP_OK) return rc;
  }
  return PGP_OK;
}

int pgp_pose_hausdorff(pgp_ctx* ctx, const float* hull_xyz, int n_hull, const float* T, int n_poses,
                       const int* pairs, int m, float* dist_max, float* dist_sum) {
  if (!ctx || n_hull < 0 || n_poses < 0 || m < 0 || (n_hull > 0 && !hull_xyz) || (n_poses > 0 && !T) ||
      (m > 0 && (!pairs || !dist_max))) {
    set_error("pgp_pose_hausdorff: bad argument");
    return PGP_EINVAL;
  }
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  std::vector<float4> hh((size_t)std::max(n_hull, 1));
  for (int i = 0; i < n_hull; ++i) hh[i] = make_float4(hull_xyz[3 * (size_t)i], hull_xyz[3 * (size_t)i + 1], hull_xyz[3 * (size_t)i + 2], 0.f);
  const size_t b_h = (hh.size() * 16 + 255) & ~(size_t)255, b_T = ((size_t)std::max(n_poses, 1) * 64 + 255) & ~(size_t)255,
               b_p = ((size_t)m * 8 + 255) & ~(size_t)255, b_o = ((size_t)m * 4 + 255) & ~(size_t)255;
  int rc = ctx->d_pre_io.ensure(b_h + b_T + b_p + 2 * b_o);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_pre_io.as<unsigned char>();
  float4* d_h = reinterpret_cast<float4*>(base);
  float* d_T = reinterpret_cast<float*>(base + b_h);
  int2* d_p = reinterpret_cast<int2*>(base + b_h + b_T);
  float* d_mx = reinterpret_cast<float*>(base + b_h + b_T + b_p);
  float* d_sm = reinterpret_cast<float*>(base + b_h + b_T + b_p + b_o);
  PGP_HIP(hipMemcpyAsync(d_h, hh.data(), (size_t)n_hull * 16, hipMemcpyHostToDevice, st));
  if (n_poses > 0) PGP_HIP(hipMemcpyAsync(d_T, T, (size_t)n_poses * 64, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_p, pairs, (size_t)m * 8, hipMemcpyHostToDevice, st));
  rc = launch_pose_hausdorff(ctx, d_h, n_hull, d_T, n_poses, d_p, m, d_mx, d_sm, st);
  if (rc != PGP_OK) return rc;
  {
    HostOut out(ctx, st);
    int rc_out;
    if ((rc_out = out.to(dist_max, d_mx, (size_t)m * 4)) != PGP_OK || (dist_sum && (rc_out = out.to(dist_sum, d_sm, (size_t)m * 4)) != PGP_OK) ||
        (rc_out = out.sync()) != PGP_OK)   // (the wait also covers hh, a stack-owned staging vector)
      return rc_out;
  }
  return PGP_OK;
}

int pgp_backproject_depth_device(pgp_ctx* ctx, const void* d_image, int raw16, const unsigned char* d_mask,
                                 int rows, int cols, const float K[9], double z_min, double z_max,
                                 float* d_xyz_out, int cap, int* n_out, void* stream) {
  if (!ctx || rows < 0 || cols < 0 || cap < 0 || !K || !n_out || (cap > 0 && !d_xyz_out) ||
      ((size_t)rows * cols > 0 && !d_image) || (size_t)rows * cols > ((size_t)1 << 30)) {
    set_error("pgp_backproject_depth_device: bad argument");
    return PGP_EINVAL;
  }
  *n_out = 0;
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx, false);
  const size_t nb = (n + 255) / 256;
  const size_t ctr_bytes = ((nb + 1) * 4 + 255) & ~(size_t)255;
  const size_t scan_bytes = ((nb / 2048 + 4) * 4 + 255) & ~(size_t)255;
  int rc = ctx->d_bp.ensure(ctr_bytes + scan_bytes + 256);
  if (rc != PGP_OK) return rc;
  uint32_t* d_ctr = ctx->d_bp.as<uint32_t>();
  uint32_t* d_scan = reinterpret_cast<uint32_t*>(ctx->d_bp.as<unsigned char>() + ctr_bytes);
  return launch_backproject(ctx, d_image, raw16 != 0, d_mask, rows, cols, K, z_min, z_max, d_ctr, d_scan, d_xyz_out, cap,
                            n_out, static_cast<hipStream_t>(stream));
}

// ---- the segment front end on device arrays (segment.hip) -----------------------------------------------------------
namespace {
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
}  // namespace

int pgp_radius_outlier_filter_device(pgp_ctx* ctx, const float* d_xyz, const float* d_nrm, int n, float radius,
                                     int min_neighbors, float* d_out_xyz, float* d_out_nrm, int* d_out_index, int cap,
                                     int* n_kept, void* stream) {
  if (!ctx || n < 0 || cap < 0 || !n_kept || !(radius > 0.f) || !std::isfinite(radius) || (n > 0 && !d_xyz) ||
      (cap > 0 && !d_out_xyz)) {
    set_error("pgp_radius_outlier_filter_device: bad argument");
    return PGP_EINVAL;
  }
  {
    const void* in[2] = {d_xyz, d_nrm};
    const void* out[3] = {d_out_xyz, d_out_nrm, d_out_index};
    const size_t out_bytes[3] = {(size_t)cap * 12, (size_t)cap * 12, (size_t)cap * 4};
    bool clash = false;
    for (int o = 0; o < 3; ++o) {
      for (int i = 0; i < 2; ++i) clash = clash || ranges_overlap(in[i], (size_t)n * 12, out[o], out_bytes[o]);
      for (int p = o + 1; p < 3; ++p) clash = clash || ranges_overlap(out[o], out_bytes[o], out[p], out_bytes[p]);
    }
    if (clash) {
      set_error("pgp_radius_outlier_filter_device: the outputs overlap the inputs or each other");
      return PGP_EINVAL;
    }
  }
  *n_kept = 0;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PGP_HIP(hipStreamSynchronize(st));   // the producer of d_xyz
  PGP_HIP(hipDeviceSynchronize());     // queued launches may still read the scene replaced below
  int rc = launch_radius_filter(ctx, d_xyz, d_nrm, n, radius, min_neighbors, d_out_xyz, d_out_nrm, d_out_index, cap, n_kept, st);
  if (rc != PGP_OK) return rc;
  return index_settled(ctx);   // the stream that waited for the temporary index has been synchronised
}

int pgp_center_device(pgp_ctx* ctx, float* d_xyz, int n, float centroid[3], void* stream) {
  if (!ctx || n <= 0 || !d_xyz || !centroid) {   // n == 0: the host helper divides by zero there
    set_error("pgp_center_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = ctx->d_seg_c.ensure(256);
  if (rc != PGP_OK) return rc;
  if ((rc = launch_center(d_xyz, n, ctx->d_seg_c.as<float>(), nullptr, st)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(centroid, ctx->d_seg_c.p, 12, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

int pgp_shift_device(pgp_ctx* ctx, float* d_xyz, int n, const float shift[3], void* stream) {
  if (!ctx || n < 0 || (n > 0 && !d_xyz) || !shift) {
    set_error("pgp_shift_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  return launch_center(d_xyz, n, nullptr, shift, static_cast<hipStream_t>(stream));
}

int pgp_weights_from_image_device(pgp_ctx* ctx, const float* d_xyz_centred, int n, const float centroid_P[3],
                                  const float K[9], const unsigned short* d_img, int rows, int cols, float* d_weights,
                                  void* stream) {
  if (!ctx || n < 0 || rows < 0 || cols < 0 || (n > 0 && (!d_xyz_centred || !d_weights)) || !centroid_P || !K ||
      ((size_t)rows * cols > 0 && !d_img)) {
    set_error("pgp_weights_from_image_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  return launch_weights_from_image(d_xyz_centred, n, centroid_P, K, d_img, rows, cols, d_weights,
                                   static_cast<hipStream_t>(stream));
}

int pgp_segment_default_options(pgp_segment_options* opt) {
  if (!opt) {
    set_error("pgp_segment_default_options: bad argument");
    return PGP_EINVAL;
  }
  opt->z_min = 0.1;             // utilities.cpp:197
  opt->z_max = 2.0;
  opt->voxel_leaf = 0.01f;      // Segmentation.cpp:235
  opt->mls_radius = 0.02f;      // Segmentation.cpp:243
  opt->filter_radius = 0.03f;   // ObjectPoseCandidateSet.cpp:30
  opt->min_neighbors = 10;      // :31
  opt->min_points = 30;         // :34
  opt->delta = 0.005f;          // super4pcs_test.cc:20
  return PGP_OK;
}

// A composition of the entry points above: every stage is the single call a caller would make, on the context's workspace.
int pgp_segment_from_depth_device(pgp_ctx* ctx, const pgp_segment_options* opt, const void* d_image, int raw16,
                                  const unsigned char* d_mask, int rows, int cols, const float K[9],
                                  const unsigned short* d_prob, int counts[4], int* installed, float centroid_P[3],
                                  void* stream) {
  if (!ctx || !opt || rows < 0 || cols < 0 || !K || !counts || !installed || !centroid_P ||
      ((size_t)rows * cols > 0 && !d_image) || (size_t)rows * cols > ((size_t)1 << 30) || !(opt->voxel_leaf > 0.f) ||
      !(opt->mls_radius > 0.f) || !(opt->filter_radius > 0.f) || !(opt->delta > 0.f) || !std::isfinite(opt->delta) ||
      opt->min_points < 0) {
    set_error("pgp_segment_from_depth_device: bad argument");
    return PGP_EINVAL;
  }
  for (int k = 0; k < 4; ++k) counts[k] = 0;
  for (int k = 0; k < 3; ++k) centroid_P[k] = 0.f;
  *installed = 0;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n_pix = (size_t)rows * cols;
  int rc;
  // 1. back-projection: the buffer holds what the last frames needed; a mask that keeps more runs the pass again
  if (ctx->d_seg_cloud.cap < 12 && (rc = ctx->d_seg_cloud.ensure(std::min<size_t>(std::max<size_t>(n_pix, 1), 65536) * 12)) != PGP_OK)
    return rc;
  int cap0 = (int)std::min<size_t>(ctx->d_seg_cloud.cap / 12, n_pix);
  rc = pgp_backproject_depth_device(ctx, d_image, raw16, d_mask, rows, cols, K, opt->z_min, opt->z_max,
                                    ctx->d_seg_cloud.as<float>(), cap0, &counts[0], stream);
  if (rc != PGP_OK) return rc;
  if (counts[0] > cap0) {
    if ((rc = ctx->d_seg_cloud.ensure((size_t)counts[0] * 12)) != PGP_OK) return rc;
    rc = pgp_backproject_depth_device(ctx, d_image, raw16, d_mask, rows, cols, K, opt->z_min, opt->z_max,
                                      ctx->d_seg_cloud.as<float>(), counts[0], &counts[0], stream);
    if (rc != PGP_OK) return rc;
  }
  // 2. voxel grid
  const int n0 = counts[0];
  if ((rc = ctx->d_seg_leaves.ensure((size_t)std::max(n0, 1) * 12)) != PGP_OK) return rc;
  rc = pgp_voxel_grid_device(ctx, ctx->d_seg_cloud.as<float>(), n0, opt->voxel_leaf, ctx->d_seg_leaves.as<float>(), n0,
                             &counts[1], stream);
  if (rc != PGP_OK) return rc;
  // 3. MLS normals; 4. filter + flip
  const int n1 = counts[1];
  Carve lay;
  const size_t r1 = (size_t)std::max(n1, 1);
  const auto p_mx = lay.add<float>(3 * r1, 256), p_mn = lay.add<float>(3 * r1, 256), p_fx = lay.add<float>(3 * r1, 256),
             p_fn = lay.add<float>(3 * r1, 256), p_w = lay.add<float>(r1, 256);
  if ((rc = lay.ensure(ctx->d_seg_rows)) != PGP_OK) return rc;
  rc = pgp_mls_normals_device(ctx, ctx->d_seg_leaves.as<float>(), n1, opt->mls_radius, lay.at(p_mx), lay.at(p_mn), nullptr,
                              nullptr, n1, &counts[2], stream);
  if (rc != PGP_OK) return rc;
  const int n2 = counts[2];
  int n3 = 0;
  if (n2 > 0) {
    rc = pgp_radius_outlier_filter_device(ctx, lay.at(p_mx), lay.at(p_mn), n2, opt->filter_radius, opt->min_neighbors,
                                          lay.at(p_fx), lay.at(p_fn), nullptr, n1, &n3, stream);
    if (rc != PGP_OK) return rc;
  }
  counts[3] = n3;
  if (n3 <= opt->min_points) {   // the node bails out here (ObjectPoseCandidateSet.cpp:34-37): no scene
    if ((rc = pgp_set_scene_device(ctx, nullptr, nullptr, nullptr, 0, opt->delta, stream)) != PGP_OK) return rc;
    ctx->has_index = false;
    return PGP_OK;
  }
  // 5. centring; 6. weights; 7. the scene
  if ((rc = pgp_center_device(ctx, lay.at(p_fx), n3, centroid_P, stream)) != PGP_OK) return rc;
  if (d_prob) {
    rc = pgp_weights_from_image_device(ctx, lay.at(p_fx), n3, centroid_P, K, d_prob, rows, cols, lay.at(p_w), stream);
    if (rc != PGP_OK) return rc;
  }
  rc = pgp_set_scene_device(ctx, lay.at(p_fx), lay.at(p_fn), d_prob ? lay.at(p_w) : nullptr, n3, opt->delta, stream);
  if (rc != PGP_OK) return rc;
  *installed = 1;
  return PGP_OK;
}

int pgp_cluster_poses_device(pgp_ctx* ctx, const float* d_T, const float* d_scores, int n_h, float best_score,
                             const float sym_deg[3], const pgp_cluster_params* params, int* d_rep_index,
                             int* d_assignment, int* n_rep, void* stream) {
  if (!ctx || n_h < 0 || !n_rep || !sym_deg || (n_h > 0 && (!d_T || !d_scores || !d_rep_index || !d_assignment))) {
    set_error("pgp_cluster_poses_device: bad argument");
    return PGP_EINVAL;
  }
  *n_rep = 0;
  if (n_h == 0) return PGP_OK;
  const pgp_cluster_params dflt = {0.5f, 10.f, 0.02f};  // HypothesisSelection.cpp:70,99
  if (!params) params = &dflt;
  CtxGuard guard(ctx, false);
  int m = 0;
  return launch_cluster(ctx, d_T, d_scores, n_h, best_score, sym_deg, params, d_rep_index, d_assignment, &m, n_rep,
                        static_cast<hipStream_t>(stream));
}

int pgp_depth_cost(pgp_ctx* ctx, const float* observed, const float* rendered, int n, int rows, int cols,
                   float threshold, float* render_score, int* counts) {
  if (!ctx || n < 0 || rows < 0 || cols < 0 || (n > 0 && (!observed || !rendered || !render_score))) {
    set_error("pgp_depth_cost: bad argument");
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t npix = (size_t)rows * cols;
  const size_t img_bytes = (npix * 4 + 15) & ~(size_t)15;
  int rc = ctx->d_depth.ensure(img_bytes * ((size_t)n + 1) + (size_t)n * 12 + 64);
  if (rc != PGP_OK) return rc;
  float* d_obs = ctx->d_depth.as<float>();
  float* d_ren = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(d_obs) + img_bytes);
  int* d_counts = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(d_ren) + (size_t)n * npix * 4 + 16);
  d_counts = reinterpret_cast<int*>(((uintptr_t)d_counts + 15) & ~(uintptr_t)15);
  if (npix > 0) {
    PGP_HIP(hipMemcpyAsync(d_obs, observed, npix * 4, hipMemcpyHostToDevice, st));
    PGP_HIP(hipMemcpyAsync(d_ren, rendered, (size_t)n * npix * 4, hipMemcpyHostToDevice, st));
  }
  rc = launch_depth_cost(ctx, d_obs, d_ren, n, (int)npix, threshold, d_counts, st);
  if (rc != PGP_OK) return rc;
  std::vector<int> hc((size_t)n * 3);
  PGP_HIP(hipMemcpyAsync(hc.data(), d_counts, hc.size() * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) {
    render_score[i] = (float)hc[3 * i] + (float)hc[3 * i + 1] - (float)hc[3 * i + 2];  // UCTState.cpp:115
    if (counts) {
      counts[3 * i] = hc[3 * i];
      counts[3 * i + 1] = hc[3 * i + 1];
      counts[3 * i + 2] = hc[3 * i + 2];
    }
  }
  return PGP_OK;
}

int pgp_depth_cost_device(pgp_ctx* ctx, const float* d_observed, const float* d_rendered, int n, int rows, int cols,
                          float threshold, int* d_counts, float* d_scores, void* stream) {
  if (!ctx || n < 0 || rows < 0 || cols < 0 || (n > 0 && (!d_observed || !d_rendered || !d_counts))) {
    set_error("pgp_depth_cost_device: bad argument");
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = launch_depth_cost(ctx, d_observed, d_rendered, n, (int)((size_t)rows * cols), threshold, d_counts, st);
  if (rc == PGP_OK && d_scores) rc = launch_cost_scores(d_counts, n, d_scores, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_render_depth_device(pgp_ctx* ctx, const float* d_vertices, int vertex_stride, int n_vert, const int* d_triangles,
                            int n_tri, const float* d_T, int n, const pgp_camera* cam, const float* d_parent,
                            size_t parent_stride, float* d_depth, void* stream) {
  if (!ctx || !cam || n < 0 || n_vert < 0 || n_tri < 0 || (n > 0 && (!d_T || !d_depth)) || (n_vert > 0 && !d_vertices)) {
    set_error("pgp_render_depth_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_render_depth(ctx, d_vertices, vertex_stride, n_vert, d_triangles, n_tri, d_T, n, cam, d_parent,
                                     parent_stride, d_depth, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_render_depth(pgp_ctx* ctx, const float* vertices, int n_vert, const int* triangles, int n_tri, const float* T,
                     int n, const pgp_camera* cam, const float* parent, float* depth) {
  if (!ctx || !cam || n < 0 || n_vert < 0 || n_tri < 0 || (n > 0 && (!T || !depth)) || (n_vert > 0 && !vertices) ||
      cam->rows <= 0 || cam->cols <= 0) {
    set_error("pgp_render_depth: bad argument");
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t n_pix = (size_t)cam->rows * cam->cols;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t off_t = up((size_t)std::max(n_vert, 1) * 12), off_T = off_t + up((size_t)std::max(n_tri, 1) * 12),
               off_p = off_T + up((size_t)n * 64), off_o = off_p + up(n_pix * 4), total = off_o + n_pix * 4 * (size_t)n;
  int rc = ctx->d_render_io.ensure(total);
  if (rc != PGP_OK) return rc;
  unsigned char* d = ctx->d_render_io.as<unsigned char>();
  if (n_vert > 0) PGP_HIP(hipMemcpyAsync(d, vertices, (size_t)n_vert * 12, hipMemcpyHostToDevice, st));
  if (triangles && n_tri > 0) PGP_HIP(hipMemcpyAsync(d + off_t, triangles, (size_t)n_tri * 12, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d + off_T, T, (size_t)n * 64, hipMemcpyHostToDevice, st));
  if (parent) PGP_HIP(hipMemcpyAsync(d + off_p, parent, n_pix * 4, hipMemcpyHostToDevice, st));
  rc = launch_render_depth(ctx, reinterpret_cast<const float*>(d), 3, n_vert,
                           triangles ? reinterpret_cast<const int*>(d + off_t) : nullptr, n_tri,
                           reinterpret_cast<const float*>(d + off_T), n, cam,
                           parent ? reinterpret_cast<const float*>(d + off_p) : nullptr, 0,
                           reinterpret_cast<float*>(d + off_o), st);
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(depth, d + off_o, n_pix * 4 * (size_t)n, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

int pgp_cluster_poses(pgp_ctx* ctx, const float* T, const float* scores, int n_h, float best_score,
                      const float sym_deg[3], const pgp_cluster_params* params, int* rep_index, int cap,
                      int* n_rep, int* assignment) {
  if (!ctx || n_h < 0 || cap < 0 || !n_rep || !sym_deg || (n_h > 0 && (!T || !scores)) || (cap > 0 && !rep_index)) {
    set_error("pgp_cluster_poses: bad argument");
    return PGP_EINVAL;
  }
  *n_rep = 0;
  if (n_h == 0) return PGP_OK;
  const pgp_cluster_params dflt = {0.5f, 10.f, 0.02f};  // HypothesisSelection.cpp:70,99
  if (!params) params = &dflt;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t nT = (size_t)n_h * 64, nS = ((size_t)n_h * 4 + 63) & ~(size_t)63;
  int rc = ctx->d_cl_io.ensure(nT + 3 * nS);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_cl_io.as<unsigned char>();
  float* d_T = reinterpret_cast<float*>(base);
  float* d_s = reinterpret_cast<float*>(base + nT);
  int* d_rep = reinterpret_cast<int*>(base + nT + nS);
  int* d_assign = reinterpret_cast<int*>(base + nT + 2 * nS);
  PGP_HIP(hipMemcpyAsync(d_T, T, nT, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_s, scores, (size_t)n_h * 4, hipMemcpyHostToDevice, st));
  int m = 0, nr = 0;
  rc = launch_cluster(ctx, d_T, d_s, n_h, best_score, sym_deg, params, d_rep, d_assign, &m, &nr, st);
  if (rc != PGP_OK) return rc;
  *n_rep = nr;
  const int n_copy = nr < cap ? nr : cap;
  HostOut out(ctx, st);
  if (n_copy > 0 && (rc = out.to(rep_index, d_rep, (size_t)n_copy * 4)) != PGP_OK) return rc;
  if (assignment && (rc = out.to(assignment, d_assign, (size_t)n_h * 4)) != PGP_OK) return rc;
  return out.sync();
}

int pgp_pose_error(pgp_ctx* ctx, const float* test, const float* gt, int n, const float sym_deg[3],
                   float* rot_err_deg, float* trans_err) {
  if (!ctx || n < 0 || !sym_deg || (n > 0 && (!test || !gt || !rot_err_deg || !trans_err))) {
    set_error("pgp_pose_error: bad argument");
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t nT = (size_t)n * 64, nS = ((size_t)n * 4 + 63) & ~(size_t)63;
  int rc = ctx->d_cl_io.ensure(2 * nT + 2 * nS);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_cl_io.as<unsigned char>();
  float* d_a = reinterpret_cast<float*>(base);
  float* d_g = reinterpret_cast<float*>(base + nT);
  float* d_r = reinterpret_cast<float*>(base + 2 * nT);
  float* d_t = reinterpret_cast<float*>(base + 2 * nT + nS);
  PGP_HIP(hipMemcpyAsync(d_a, test, nT, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_g, gt, nT, hipMemcpyHostToDevice, st));
  rc = launch_pose_error(ctx, d_a, d_g, n, sym_deg, d_r, d_t, st);
  if (rc != PGP_OK) return rc;
  {
    HostOut out(ctx, st);
    int rc_out;
    if ((rc_out = out.to(rot_err_deg, d_r, (size_t)n * 4)) != PGP_OK || (rc_out = out.to(trans_err, d_t, (size_t)n * 4)) != PGP_OK ||
        (rc_out = out.sync()) != PGP_OK)
      return rc_out;
  }
  return PGP_OK;
}

int pgp_set_kernel_timing(pgp_ctx* ctx, int enable) {
  if (!ctx) {
    set_error("pgp_set_kernel_timing: ctx is NULL");
    return PGP_EINVAL;
  }
  ctx->timing = enable > 0 ? enable : 0;
  ctx->timing_seq = 0;
  return PGP_OK;
}

int pgp_get_kernel_timing(pgp_ctx* ctx, int* launches, float* total_ms, int reset) {
  if (!ctx || !launches || !total_ms) {
    set_error("pgp_get_kernel_timing: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  float sum = 0.f;
  for (size_t k = 0; k + 1 < ctx->ev_used; k += 2) {
    PGP_HIP(hipEventSynchronize(ctx->ev[k + 1]));
    float ms = 0.f;
    PGP_HIP(hipEventElapsedTime(&ms, ctx->ev[k], ctx->ev[k + 1]));
    sum += ms;
  }
  *launches = (int)(ctx->ev_used / 2);
  *total_ms = sum;
  if (reset) ctx->ev_used = 0;
  return PGP_OK;
}

int pgp_get_index_info(pgp_ctx* ctx, pgp_index_info* info) {
  if (!ctx || !info) {
    set_error("pgp_get_index_info: bad argument");
    return PGP_EINVAL;
  }
  std::memset(info, 0, sizeof *info);
  info->n_scene = ctx->nP;
  info->n_model = ctx->nQ;
  if (ctx->has_index) {
    CtxGuard guard(ctx);
    const int rc = finish_index(ctx);   // a build on the side stream: its counts are known when it is through
    if (rc != PGP_OK) return rc;
    info->grid_nx = ctx->grid.nx;
    info->grid_ny = ctx->grid.ny;
    info->grid_nz = ctx->grid.nz;
    info->cell_size = ctx->grid.h;
    info->delta = ctx->delta;
    info->n_cells = ctx->n_cells;
    info->n_candidates = ctx->n_cand;
    info->n_occupied = ctx->n_occ;
    const size_t table = ctx->grid.sparse ? ((size_t)ctx->grid.tab_mask + 1) * 16
                                          : (size_t)ctx->grid.nbx * ctx->grid.nby * ctx->grid.nbz * 8;
    info->bytes_index = (long long)(table + (size_t)ctx->n_occ * 8 + (size_t)ctx->n_cand * 16);
    info->sparse = ctx->grid.sparse;
    info->n_blocks = ctx->grid.sparse ? ctx->n_blocks : (long long)ctx->grid.nbx * ctx->grid.nby * ctx->grid.nbz;
    info->build_ms = ctx->build_ms;
  }
  return PGP_OK;
}

}  // extern "C"

// ---- table-plane removal (plane.hip) ----------------------------------------------------------------------------
namespace {
bool plane_options_ok(const pgp_plane_options* o, const char* who) {
  if (!o || !(o->threshold > 0.f) || !std::isfinite(o->threshold) || o->max_iterations < 1 ||
      o->max_iterations >= plane_max_candidates() || !(o->probability > 0.0 && o->probability < 1.0) ||
      (o->stop != PGP_PLANE_STOP_ADAPTIVE && o->stop != PGP_PLANE_STOP_ALL)) {
    set_error("%s: bad options (threshold > 0, 1 <= max_iterations < %d, 0 < probability < 1, stop 0 or 1)", who,
              plane_max_candidates());
    return false;
  }
  return true;
}

// the double of a float's shortest decimal form (0.005f -> 0.005): the literal a float option stands for
double shortest_decimal(float f) {
  char buf[48];
  for (int p = 1; p <= 9; ++p) {
    std::snprintf(buf, sizeof buf, "%.*g", p, (double)f);
    if (std::strtof(buf, nullptr) == f) return std::strtod(buf, nullptr);
  }
  return (double)f;
}
}  // namespace

extern "C" {

int pgp_plane_default_options(pgp_plane_options* opt) {
  if (!opt) {
    set_error("pgp_plane_default_options: null");
    return PGP_EINVAL;
  }
  opt->threshold = 0.005f;
  opt->max_iterations = 1000;
  opt->probability = 0.99;
  opt->stop = PGP_PLANE_STOP_ADAPTIVE;
  opt->optimize = 1;
  opt->seed = 0;
  return PGP_OK;
}

int pgp_fit_plane_device(pgp_ctx* ctx, const float* d_xyz, int n, const pgp_plane_options* opt, const int* d_samples,
                         int n_samples, float* d_coeff, unsigned char* d_inliers, int* d_n_inliers,
                         pgp_plane_info* d_info, void* stream) {
  if (!ctx || n < 3 || !d_xyz || !d_coeff || !d_n_inliers || (d_samples && (n_samples < 1 || n_samples > plane_max_candidates()))) {
    set_error("pgp_fit_plane_device: bad argument (n = %d >= 3, 1 <= n_samples <= %d)", n, plane_max_candidates());
    return PGP_EINVAL;
  }
  if (!plane_options_ok(opt, "pgp_fit_plane_device")) return PGP_EINVAL;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_fit_plane(ctx, d_xyz, n, opt, d_samples, n_samples, d_coeff, d_inliers, d_n_inliers, d_info, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_fit_plane(pgp_ctx* ctx, const float* xyz, int n, const pgp_plane_options* opt, const int* samples, int n_samples,
                  float coeff[4], unsigned char* inliers, int* n_inliers, pgp_plane_info* info) {
  if (!ctx || n < 3 || !xyz || !coeff || !n_inliers || (samples && (n_samples < 1 || n_samples > plane_max_candidates()))) {
    set_error("pgp_fit_plane: bad argument (n = %d >= 3, 1 <= n_samples <= %d)", n, plane_max_candidates());
    return PGP_EINVAL;
  }
  if (!plane_options_ok(opt, "pgp_fit_plane")) return PGP_EINVAL;
  for (size_t i = 0; i < (size_t)n * 3; ++i)
    if (!std::isfinite(xyz[i])) {
      set_error("pgp_fit_plane: point %zu is not finite", i / 3);
      return PGP_EINVAL;
    }
  if (samples)
    for (size_t i = 0; i < (size_t)n_samples * 3; ++i)
      if (samples[i] < 0 || samples[i] >= n) {
        set_error("pgp_fit_plane: sample %zu names point %d of %d", i / 3, samples[i], n);
        return PGP_EINVAL;
      }
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t b_xyz = ((size_t)n * 12 + 255) & ~(size_t)255, b_s = samples ? ((size_t)n_samples * 12 + 255) & ~(size_t)255 : 0,
               b_m = ((size_t)n + 255) & ~(size_t)255;
  int rc = ctx->d_plane_io.ensure(b_xyz + b_s + b_m + 512);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_plane_io.as<unsigned char>();
  float* d_xyz = reinterpret_cast<float*>(base);
  int* d_s = samples ? reinterpret_cast<int*>(base + b_xyz) : nullptr;
  unsigned char* d_m = base + b_xyz + b_s;
  float* d_c = reinterpret_cast<float*>(base + b_xyz + b_s + b_m);
  int* d_n = reinterpret_cast<int*>(base + b_xyz + b_s + b_m + 64);
  pgp_plane_info* d_i = reinterpret_cast<pgp_plane_info*>(base + b_xyz + b_s + b_m + 128);
  PGP_HIP(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
  if (samples) PGP_HIP(hipMemcpyAsync(d_s, samples, (size_t)n_samples * 12, hipMemcpyHostToDevice, st));
  if ((rc = launch_fit_plane(ctx, d_xyz, n, opt, d_s, n_samples, d_c, inliers ? d_m : nullptr, d_n, d_i, st)) != PGP_OK)
    return rc;
  pgp_plane_info h_info;
  HostOut out(ctx, st);
  if ((rc = out.to(coeff, d_c, 16)) != PGP_OK || (rc = out.to(n_inliers, d_n, 4)) != PGP_OK ||
      (rc = out.to(&h_info, d_i, sizeof h_info)) != PGP_OK || (inliers && (rc = out.to(inliers, d_m, (size_t)n)) != PGP_OK) ||
      (rc = out.sync()) != PGP_OK)
    return rc;
  if (info) *info = h_info;
  return PGP_OK;
}

int pgp_mask_plane_depth_device(pgp_ctx* ctx, void* d_image, int raw16, int rows, int cols, const float K[9],
                                const float coeff[4], double threshold, int* d_n_masked, void* stream) {
  if (!ctx || rows < 0 || cols < 0 || !K || !coeff || ((size_t)rows * cols > 0 && !d_image) ||
      (size_t)rows * cols > ((size_t)1 << 30) || !(threshold > 0.0) || !std::isfinite(threshold)) {
    set_error("pgp_mask_plane_depth_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_mask_plane_depth(ctx, d_image, raw16 != 0, rows, cols, K, coeff, nullptr, threshold, d_n_masked, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_mask_plane_depth(pgp_ctx* ctx, void* image, int raw16, int rows, int cols, const float K[9], const float coeff[4],
                         double threshold, int* n_masked) {
  if (!ctx || rows < 0 || cols < 0 || !K || !coeff || ((size_t)rows * cols > 0 && !image) ||
      (size_t)rows * cols > ((size_t)1 << 30) || !(threshold > 0.0) || !std::isfinite(threshold)) {
    set_error("pgp_mask_plane_depth: bad argument");
    return PGP_EINVAL;
  }
  if (n_masked) *n_masked = 0;
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t px = raw16 ? 2 : 4, b_img = (n * px + 255) & ~(size_t)255;
  int rc = ctx->d_plane_io.ensure(b_img + 256);
  if (rc != PGP_OK) return rc;
  unsigned char* d_img = ctx->d_plane_io.as<unsigned char>();
  int* d_n = reinterpret_cast<int*>(d_img + b_img);
  PGP_HIP(hipMemcpyAsync(d_img, image, n * px, hipMemcpyHostToDevice, st));
  if ((rc = launch_mask_plane_depth(ctx, d_img, raw16 != 0, rows, cols, K, coeff, nullptr, threshold, d_n, st)) != PGP_OK)
    return rc;
  PGP_HIP(hipMemcpyAsync(image, d_img, n * px, hipMemcpyDeviceToHost, st));
  int cnt = 0;
  PGP_HIP(hipMemcpyAsync(&cnt, d_n, 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  if (n_masked) *n_masked = cnt;
  return PGP_OK;
}

int pgp_remove_table(pgp_ctx* ctx, void* image, int raw16, int rows, int cols, const float K[9], float leaf,
                     const pgp_plane_options* opt, float coeff[4], int* n_masked) {
  if (!ctx || rows < 0 || cols < 0 || !K || ((size_t)rows * cols > 0 && !image) || (size_t)rows * cols > ((size_t)1 << 30) ||
      !(leaf > 0.f) || !std::isfinite(leaf)) {
    set_error("pgp_remove_table: bad argument");
    return PGP_EINVAL;
  }
  if (!plane_options_ok(opt, "pgp_remove_table")) return PGP_EINVAL;
  if (n_masked) *n_masked = 0;
  if (coeff) coeff[0] = coeff[1] = coeff[2] = coeff[3] = 0.f;
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  // image | cloud (n x 3) | voxels (n x 3) | back-projection counters + scan scratch | coeff, counts, info
  const size_t px = raw16 ? 2 : 4, b_img = (n * px + 255) & ~(size_t)255, b_xyz = (n * 12 + 255) & ~(size_t)255;
  const size_t nb = (n + 255) / 256, b_ctr = ((nb + 1) * 4 + 255) & ~(size_t)255, b_scan = ((nb / 2048 + 4) * 4 + 255) & ~(size_t)255;
  int rc = ctx->d_plane_io.ensure(b_img + 2 * b_xyz + b_ctr + b_scan + 512);
  if (rc != PGP_OK) return rc;
  unsigned char* base = ctx->d_plane_io.as<unsigned char>();
  void* d_img = base;
  float* d_cloud = reinterpret_cast<float*>(base + b_img);
  float* d_vox = reinterpret_cast<float*>(base + b_img + b_xyz);
  uint32_t* d_ctr = reinterpret_cast<uint32_t*>(base + b_img + 2 * b_xyz);
  uint32_t* d_scan = reinterpret_cast<uint32_t*>(base + b_img + 2 * b_xyz + b_ctr);
  unsigned char* tail = base + b_img + 2 * b_xyz + b_ctr + b_scan;
  float* d_c = reinterpret_cast<float*>(tail);
  int* d_cnt = reinterpret_cast<int*>(tail + 64);   // [0] inliers, [1] masked
  pgp_plane_info* d_i = reinterpret_cast<pgp_plane_info*>(tail + 128);
  PGP_HIP(hipMemcpyAsync(d_img, image, n * px, hipMemcpyHostToDevice, st));
  int n_pts = 0, n_vox = 0;
  if ((rc = launch_backproject(ctx, d_img, raw16 != 0, nullptr, rows, cols, K, 0.1, 2.0, d_ctr, d_scan, d_cloud, (int)n, &n_pts,
                               st)) != PGP_OK)
    return rc;
  if ((rc = launch_voxel_grid(ctx, d_cloud, n_pts, leaf, d_vox, (int)n, &n_vox, st)) != PGP_OK) return rc;
  if (n_vox < 3) {   // nothing to fit: the image stays as it is
    PGP_HIP(hipStreamSynchronize(st));
    return PGP_OK;
  }
  if ((rc = launch_fit_plane(ctx, d_vox, n_vox, opt, nullptr, 0, d_c, nullptr, d_cnt, d_i, st)) != PGP_OK) return rc;
  if ((rc = launch_mask_plane_depth(ctx, d_img, raw16 != 0, rows, cols, K, nullptr, d_c, shortest_decimal(opt->threshold),
                                    d_cnt + 1, st)) != PGP_OK)
    return rc;
  PGP_HIP(hipMemcpyAsync(image, d_img, n * px, hipMemcpyDeviceToHost, st));
  float h_c[4];
  int h_cnt[2];
  PGP_HIP(hipMemcpyAsync(h_c, d_c, 16, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipMemcpyAsync(h_cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  if (coeff) std::memcpy(coeff, h_c, 16);
  if (n_masked) *n_masked = h_cnt[1];
  return PGP_OK;
}

}  // extern "C"

// ---- object proposals: connected components of a depth image (components.hip) ---------------------------------------
namespace {
bool components_args_ok(const pgp_ctx* ctx, const pgp_components_options* opt, const void* image, const unsigned char* mask,
                        int raw16, int rows, int cols, const float* K, const int* roots, const int* ids,
                        const pgp_component_info* info, int cap, const int* counts, const char* who) {
  if (!ctx || !opt || rows < 0 || cols < 0 || !K || !counts || cap < 0 || (cap > 0 && !info) ||
      ((size_t)rows * cols > 0 && !image) || (size_t)rows * cols > ((size_t)1 << 30)) {
    set_error("%s: bad argument (cap >= 0, info with cap > 0, rows * cols <= 2^30)", who);
    return false;
  }
  if (!(opt->tolerance > 0.f) || !std::isfinite(opt->tolerance) || (opt->connectivity != 4 && opt->connectivity != 8) ||
      opt->min_pixels < 1) {
    set_error("%s: bad options (tolerance > 0 and finite, connectivity 4 or 8, min_pixels >= 1)", who);
    return false;
  }
  const size_t n = (size_t)rows * cols;
  const void* in[2] = {image, mask};
  const size_t in_bytes[2] = {n * (raw16 ? 2 : 4), n};
  const void* out[4] = {roots, ids, info, counts};
  const size_t out_bytes[4] = {n * 4, n * 4, (size_t)cap * sizeof(pgp_component_info), 12};
  bool clash = false;
  for (int o = 0; o < 4; ++o) {
    for (int i = 0; i < 2; ++i) clash = clash || ranges_overlap(in[i], in_bytes[i], out[o], out_bytes[o]);
    for (int p = o + 1; p < 4; ++p) clash = clash || ranges_overlap(out[o], out_bytes[o], out[p], out_bytes[p]);
  }
  if (clash) {
    set_error("%s: the outputs overlap the inputs or each other", who);
    return false;
  }
  return true;
}

bool assign_args_ok(const pgp_ctx* ctx, const int* ids, const void* classes, int class_bytes, int rows, int cols,
                    const int* class_values, int n_objects, const int* component, const int* pixels_in,
                    const int* pixels_total, const int* group, const char* who) {
  if (!ctx || rows < 0 || cols < 0 || (size_t)rows * cols > ((size_t)1 << 30) || (class_bytes != 1 && class_bytes != 2) ||
      n_objects < 1 || n_objects > kAssignMaxObjects || !class_values || !component || !pixels_in || !pixels_total || !group ||
      ((size_t)rows * cols > 0 && (!ids || !classes))) {
    set_error("%s: bad argument (class_bytes 1 or 2, 1 <= n_objects <= %d, rows * cols <= 2^30)", who, kAssignMaxObjects);
    return false;
  }
  const size_t n = (size_t)rows * cols, row = (size_t)n_objects * 4;
  const void* in[3] = {ids, classes, class_values};
  const size_t in_bytes[3] = {n * 4, n * (size_t)class_bytes, row};
  const void* out[4] = {component, pixels_in, pixels_total, group};
  bool clash = false;
  for (int o = 0; o < 4; ++o) {
    for (int i = 0; i < 3; ++i) clash = clash || ranges_overlap(in[i], in_bytes[i], out[o], row);
    for (int p = o + 1; p < 4; ++p) clash = clash || ranges_overlap(out[o], row, out[p], row);
  }
  if (clash) {
    set_error("%s: the outputs overlap the inputs or each other", who);
    return false;
  }
  return true;
}

// component 0 is a group of its own; equal non-zero components share one; numbered in the order of their first object
void groups_of(const int* component, int n_objects, int* group) {
  int next = 0;
  for (int o = 0; o < n_objects; ++o) {
    int g = -1;
    for (int p = 0; p < o && g < 0; ++p)
      if (component[o] != 0 && component[p] == component[o]) g = group[p];
    group[o] = g >= 0 ? g : next++;
  }
}

int assign_finish(const int* h_result, int n_objects, int* component, int* pixels_in, int* pixels_total, int* group,
                  const char* who) {
  if (h_result[3 * n_objects] != 0) {
    set_error("%s: an id outside [0, min(rows * cols, %d)]", who, kAssignMaxId);
    return PGP_EINVAL;
  }
  for (int o = 0; o < n_objects; ++o) {
    component[o] = h_result[3 * o];
    pixels_in[o] = h_result[3 * o + 1];
    pixels_total[o] = h_result[3 * o + 2];
  }
  groups_of(component, n_objects, group);
  return PGP_OK;
}
}  // namespace

extern "C" {

int pgp_components_default_options(pgp_components_options* opt) {
  if (!opt) {
    set_error("pgp_components_default_options: null");
    return PGP_EINVAL;
  }
  opt->z_min = 0.1;
  opt->z_max = 2.0;
  opt->tolerance = 0.01f;
  opt->connectivity = 4;
  opt->min_pixels = 500;
  opt->max_pixels = 0;
  return PGP_OK;
}

int pgp_depth_components_device(pgp_ctx* ctx, const pgp_components_options* opt, const void* d_image, int raw16,
                                const unsigned char* d_mask, int rows, int cols, const float K[9], int* d_roots, int* d_ids,
                                pgp_component_info* d_info, int cap, int* d_counts, void* stream) {
  if (!components_args_ok(ctx, opt, d_image, d_mask, raw16, rows, cols, K, d_roots, d_ids, d_info, cap, d_counts,
                          "pgp_depth_components_device"))
    return PGP_EINVAL;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_depth_components(ctx, opt, d_image, raw16 != 0, d_mask, rows, cols, K, d_roots, d_ids, d_info, cap,
                                         d_counts, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_depth_components(pgp_ctx* ctx, const pgp_components_options* opt, const void* image, int raw16,
                         const unsigned char* mask, int rows, int cols, const float K[9], int* roots, int* ids,
                         pgp_component_info* info, int cap, int counts[3]) {
  if (!components_args_ok(ctx, opt, image, mask, raw16, rows, cols, K, roots, ids, info, cap, counts, "pgp_depth_components"))
    return PGP_EINVAL;
  counts[0] = counts[1] = counts[2] = 0;
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t rows_cap = std::min((size_t)cap, n / (size_t)opt->min_pixels);   // info rows the device can write
  Carve cv;
  const auto c_img = cv.add<unsigned char>(n * (raw16 ? 2 : 4), 256), c_mask = cv.add<unsigned char>(mask ? n : 0, 256);
  const auto c_roots = cv.add<int>(roots ? n : 0, 256), c_ids = cv.add<int>(ids ? n : 0, 256);
  const auto c_info = cv.add<pgp_component_info>(rows_cap, 256);
  const auto c_counts = cv.add<int>(3, 256);
  cv.pad(256);
  int rc = cv.ensure(ctx->d_cc_io);
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(cv.at(c_img), image, c_img.bytes(), hipMemcpyHostToDevice, st));
  if (mask) PGP_HIP(hipMemcpyAsync(cv.at(c_mask), mask, n, hipMemcpyHostToDevice, st));
  if ((rc = launch_depth_components(ctx, opt, cv.at(c_img), raw16 != 0, mask ? cv.at(c_mask) : nullptr, rows, cols, K,
                                    roots ? cv.at(c_roots) : nullptr, ids ? cv.at(c_ids) : nullptr,
                                    rows_cap ? cv.at(c_info) : nullptr, (int)rows_cap, cv.at(c_counts), st)) != PGP_OK)
    return rc;
  int h_counts[3] = {0, 0, 0};
  if (roots) PGP_HIP(hipMemcpyAsync(roots, cv.at(c_roots), n * 4, hipMemcpyDeviceToHost, st));
  if (ids) PGP_HIP(hipMemcpyAsync(ids, cv.at(c_ids), n * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipMemcpyAsync(h_counts, cv.at(c_counts), 12, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  const size_t written = std::min((size_t)h_counts[0], rows_cap);   // rows beyond the kept count stay as the caller left them
  if (written) {
    PGP_HIP(hipMemcpyAsync(info, cv.at(c_info), written * sizeof(pgp_component_info), hipMemcpyDeviceToHost, st));
    PGP_HIP(hipStreamSynchronize(st));
  }
  std::memcpy(counts, h_counts, 12);
  return PGP_OK;
}

int pgp_component_mask_device(pgp_ctx* ctx, const int* d_ids, int rows, int cols, int id, unsigned char* d_mask, void* stream) {
  const size_t n = rows >= 0 && cols >= 0 ? (size_t)rows * cols : 0;
  if (!ctx || rows < 0 || cols < 0 || n > ((size_t)1 << 30) || (n > 0 && (!d_ids || !d_mask)) ||
      ranges_overlap(d_ids, n * 4, d_mask, n)) {
    set_error("pgp_component_mask_device: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_component_mask(d_ids, n, id, d_mask, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_component_mask(pgp_ctx* ctx, const int* ids, int rows, int cols, int id, unsigned char* mask) {
  const size_t n = rows >= 0 && cols >= 0 ? (size_t)rows * cols : 0;
  if (!ctx || rows < 0 || cols < 0 || n > ((size_t)1 << 30) || (n > 0 && (!ids || !mask)) || ranges_overlap(ids, n * 4, mask, n)) {
    set_error("pgp_component_mask: bad argument");
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  Carve cv;
  const auto c_ids = cv.add<int>(n, 256);
  const auto c_mask = cv.add<unsigned char>(n, 256);
  cv.pad(256);
  int rc = cv.ensure(ctx->d_cc_io);
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(cv.at(c_ids), ids, n * 4, hipMemcpyHostToDevice, st));
  if ((rc = launch_component_mask(cv.at(c_ids), n, id, cv.at(c_mask), st)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(mask, cv.at(c_mask), n, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

int pgp_assign_masks_to_components_device(pgp_ctx* ctx, const int* d_ids, const void* d_classes, int class_bytes, int rows,
                                          int cols, const int* class_values, int n_objects, int* component, int* pixels_in,
                                          int* pixels_total, int* group, void* stream) {
  const char* who = "pgp_assign_masks_to_components_device";
  if (!assign_args_ok(ctx, d_ids, d_classes, class_bytes, rows, cols, class_values, n_objects, component, pixels_in,
                      pixels_total, group, who))
    return PGP_EINVAL;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = ctx->d_cc_io.ensure(256 + (3 * (size_t)kAssignMaxObjects + 1) * 4);
  if (rc != PGP_OK) return rc;
  int* d_result = ctx->d_cc_io.as<int>();
  if ((rc = launch_assign_masks(ctx, d_ids, d_classes, class_bytes, (size_t)rows * cols, class_values, n_objects, d_result,
                                st)) != PGP_OK)
    return rc;
  int h_result[3 * kAssignMaxObjects + 1];
  PGP_HIP(hipMemcpyAsync(h_result, d_result, (3 * (size_t)n_objects + 1) * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return assign_finish(h_result, n_objects, component, pixels_in, pixels_total, group, who);
}

int pgp_assign_masks_to_components(pgp_ctx* ctx, const int* ids, const void* classes, int class_bytes, int rows, int cols,
                                   const int* class_values, int n_objects, int* component, int* pixels_in, int* pixels_total,
                                   int* group) {
  const char* who = "pgp_assign_masks_to_components";
  if (!assign_args_ok(ctx, ids, classes, class_bytes, rows, cols, class_values, n_objects, component, pixels_in, pixels_total,
                      group, who))
    return PGP_EINVAL;
  const size_t n = (size_t)rows * cols;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  Carve cv;
  const auto c_res = cv.add<int>(3 * (size_t)kAssignMaxObjects + 1, 256);
  const auto c_ids = cv.add<int>(n, 256);
  const auto c_cls = cv.add<unsigned char>(n * (size_t)class_bytes, 256);
  cv.pad(256);
  int rc = cv.ensure(ctx->d_cc_io);
  if (rc != PGP_OK) return rc;
  if (n > 0) {
    PGP_HIP(hipMemcpyAsync(cv.at(c_ids), ids, n * 4, hipMemcpyHostToDevice, st));
    PGP_HIP(hipMemcpyAsync(cv.at(c_cls), classes, n * (size_t)class_bytes, hipMemcpyHostToDevice, st));
  }
  if ((rc = launch_assign_masks(ctx, cv.at(c_ids), cv.at(c_cls), class_bytes, n, class_values, n_objects, cv.at(c_res), st)) !=
      PGP_OK)
    return rc;
  int h_result[3 * kAssignMaxObjects + 1];
  PGP_HIP(hipMemcpyAsync(h_result, cv.at(c_res), (3 * (size_t)n_objects + 1) * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return assign_finish(h_result, n_objects, component, pixels_in, pixels_total, group, who);
}

}  // extern "C"

// ---- touching objects: normals, concave-crease mask, cores + growing (depth_crease.hip) ------------------------------
namespace {
bool crease_options_ok(const pgp_crease_options* co, const char* who) {
  if (!co || co->normal_step < 1 || co->normal_step > 8 || co->smooth_radius < 0 || co->smooth_radius > 4 ||
      co->crease_step < 1 || co->crease_step > 8 || !(co->concavity >= 0.f) || !std::isfinite(co->concavity) ||
      co->grow_passes < 0 || co->grow_passes > 64) {
    set_error("%s: bad crease options (normal_step, crease_step 1..8, smooth_radius 0..4, concavity >= 0 and finite, "
              "grow_passes 0..64)", who);
    return false;
  }
  return true;
}

// image, mask, shape and options as pgp_depth_components checks them, and one output of out_bytes (+ an optional count)
bool crease_args_ok(const pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* co, const void* image,
                    const unsigned char* mask, int raw16, int rows, int cols, const float* K, const void* out,
                    size_t bytes_per_pixel, const int* count, bool want_count, const char* who) {
  int none[3];
  if (!components_args_ok(ctx, opt, image, mask, raw16, rows, cols, K, nullptr, nullptr, nullptr, 0, none, who) ||
      !crease_options_ok(co, who))
    return false;
  const size_t n = (size_t)rows * cols;
  if ((n > 0 && !out) || (want_count && !count)) {
    set_error("%s: null output", who);
    return false;
  }
  const size_t out_bytes = n * bytes_per_pixel, img_bytes = n * (raw16 ? 2 : 4);
  if (ranges_overlap(image, img_bytes, out, out_bytes) || ranges_overlap(mask, n, out, out_bytes) ||
      (want_count && (ranges_overlap(image, img_bytes, count, 4) || ranges_overlap(mask, n, count, 4) ||
                      ranges_overlap(out, out_bytes, count, 4)))) {
    set_error("%s: the outputs overlap the inputs or each other", who);
    return false;
  }
  return true;
}

bool objects_args_ok(const pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* co, const void* image,
                     const unsigned char* mask, int raw16, int rows, int cols, const float* K, const int* roots, const int* ids,
                     const pgp_component_info* info, int cap, const int* counts, const char* who) {
  if (!components_args_ok(ctx, opt, image, mask, raw16, rows, cols, K, roots, ids, info, cap, counts, who) ||
      !crease_options_ok(co, who))
    return false;
  // counts[3], counts[4]: the two words pgp_depth_components does not have
  const size_t n = (size_t)rows * cols;
  const void* other[5] = {image, mask, roots, ids, info};
  const size_t other_bytes[5] = {n * (raw16 ? 2 : 4), n, n * 4, n * 4, (size_t)cap * sizeof(pgp_component_info)};
  for (int k = 0; k < 5; ++k)
    if (ranges_overlap(other[k], other_bytes[k], counts + 3, 8)) {
      set_error("%s: the outputs overlap the inputs or each other", who);
      return false;
    }
  return true;
}

// image (and mask) of a host-pointer call into the staging buffer, in front of whatever the call adds to `cv`
struct StagedImage {
  Carve::Piece<unsigned char> img, mask;
  StagedImage(Carve& cv, size_t n, int raw16, bool has_mask) {
    img = cv.add<unsigned char>(n * (raw16 ? 2 : 4), 256);
    mask = cv.add<unsigned char>(has_mask ? n : 0, 256);
  }
  int upload(const Carve& cv, const void* image, const unsigned char* m, size_t n, hipStream_t st) const {
    PGP_HIP(hipMemcpyAsync(cv.at(img), image, img.bytes(), hipMemcpyHostToDevice, st));
    if (m) PGP_HIP(hipMemcpyAsync(cv.at(mask), m, n, hipMemcpyHostToDevice, st));
    return PGP_OK;
  }
};
}  // namespace

extern "C" {

int pgp_crease_default_options(pgp_crease_options* opt) {
  if (!opt) {
    set_error("pgp_crease_default_options: null");
    return PGP_EINVAL;
  }
  opt->normal_step = 3;
  opt->smooth_radius = 2;
  opt->crease_step = 4;
  opt->concavity = 0.06f;
  opt->grow_passes = 12;
  return PGP_OK;
}

int pgp_depth_normals_device(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease,
                             const void* d_image, int raw16, const unsigned char* d_mask, int rows, int cols, const float K[9],
                             float* d_normals, void* stream) {
  if (!crease_args_ok(ctx, opt, crease, d_image, d_mask, raw16, rows, cols, K, d_normals, 16, nullptr, false,
                      "pgp_depth_normals_device"))
    return PGP_EINVAL;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_depth_normals(opt, crease, d_image, raw16 != 0, d_mask, rows, cols, K, d_normals, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_depth_normals(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease, const void* image,
                      int raw16, const unsigned char* mask, int rows, int cols, const float K[9], float* normals) {
  if (!crease_args_ok(ctx, opt, crease, image, mask, raw16, rows, cols, K, normals, 16, nullptr, false, "pgp_depth_normals"))
    return PGP_EINVAL;
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  Carve cv;
  const StagedImage in(cv, n, raw16, mask != nullptr);
  const auto c_out = cv.add<float>(4 * n, 256);
  cv.pad(256);
  int rc = cv.ensure(ctx->d_cc_io);
  if (rc != PGP_OK || (rc = in.upload(cv, image, mask, n, st)) != PGP_OK) return rc;
  if ((rc = launch_depth_normals(opt, crease, cv.at(in.img), raw16 != 0, mask ? cv.at(in.mask) : nullptr, rows, cols, K,
                                 cv.at(c_out), st)) != PGP_OK)
    return rc;
  PGP_HIP(hipMemcpyAsync(normals, cv.at(c_out), c_out.bytes(), hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

int pgp_depth_crease_mask_device(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease,
                                 const void* d_image, int raw16, const unsigned char* d_mask, int rows, int cols,
                                 const float K[9], unsigned char* d_keep, int* d_n_crease, void* stream) {
  if (!crease_args_ok(ctx, opt, crease, d_image, d_mask, raw16, rows, cols, K, d_keep, 1, d_n_crease, true,
                      "pgp_depth_crease_mask_device"))
    return PGP_EINVAL;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_depth_crease_mask(ctx, opt, crease, d_image, raw16 != 0, d_mask, rows, cols, K, d_keep, d_n_crease, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_depth_crease_mask(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease, const void* image,
                          int raw16, const unsigned char* mask, int rows, int cols, const float K[9], unsigned char* keep,
                          int* n_crease) {
  if (!crease_args_ok(ctx, opt, crease, image, mask, raw16, rows, cols, K, keep, 1, n_crease, true, "pgp_depth_crease_mask"))
    return PGP_EINVAL;
  *n_crease = 0;
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  Carve cv;
  const StagedImage in(cv, n, raw16, mask != nullptr);
  const auto c_keep = cv.add<unsigned char>(n, 256);
  const auto c_count = cv.add<int>(1, 256);
  cv.pad(256);
  int rc = cv.ensure(ctx->d_cc_io);
  if (rc != PGP_OK || (rc = in.upload(cv, image, mask, n, st)) != PGP_OK) return rc;
  if ((rc = launch_depth_crease_mask(ctx, opt, crease, cv.at(in.img), raw16 != 0, mask ? cv.at(in.mask) : nullptr, rows, cols, K,
                                     cv.at(c_keep), cv.at(c_count), st)) != PGP_OK)
    return rc;
  int h_count = 0;
  PGP_HIP(hipMemcpyAsync(keep, cv.at(c_keep), n, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipMemcpyAsync(&h_count, cv.at(c_count), 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  *n_crease = h_count;
  return PGP_OK;
}

int pgp_depth_objects_device(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease,
                             const void* d_image, int raw16, const unsigned char* d_mask, int rows, int cols, const float K[9],
                             int* d_roots, int* d_ids, pgp_component_info* d_info, int cap, int* d_counts, void* stream) {
  if (!objects_args_ok(ctx, opt, crease, d_image, d_mask, raw16, rows, cols, K, d_roots, d_ids, d_info, cap, d_counts,
                       "pgp_depth_objects_device"))
    return PGP_EINVAL;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = launch_depth_objects(ctx, opt, crease, d_image, raw16 != 0, d_mask, rows, cols, K, d_roots, d_ids, d_info, cap,
                                      d_counts, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_depth_objects(pgp_ctx* ctx, const pgp_components_options* opt, const pgp_crease_options* crease, const void* image,
                      int raw16, const unsigned char* mask, int rows, int cols, const float K[9], int* roots, int* ids,
                      pgp_component_info* info, int cap, int counts[5]) {
  if (!objects_args_ok(ctx, opt, crease, image, mask, raw16, rows, cols, K, roots, ids, info, cap, counts, "pgp_depth_objects"))
    return PGP_EINVAL;
  std::memset(counts, 0, 20);
  const size_t n = (size_t)rows * cols;
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t rows_cap = std::min((size_t)cap, n / (size_t)opt->min_pixels);   // info rows the device can write
  Carve cv;
  const StagedImage in(cv, n, raw16, mask != nullptr);
  const auto c_roots = cv.add<int>(roots ? n : 0, 256), c_ids = cv.add<int>(ids ? n : 0, 256);
  const auto c_info = cv.add<pgp_component_info>(rows_cap, 256);
  const auto c_counts = cv.add<int>(5, 256);
  cv.pad(256);
  int rc = cv.ensure(ctx->d_cc_io);
  if (rc != PGP_OK || (rc = in.upload(cv, image, mask, n, st)) != PGP_OK) return rc;
  if ((rc = launch_depth_objects(ctx, opt, crease, cv.at(in.img), raw16 != 0, mask ? cv.at(in.mask) : nullptr, rows, cols, K,
                                 roots ? cv.at(c_roots) : nullptr, ids ? cv.at(c_ids) : nullptr,
                                 rows_cap ? cv.at(c_info) : nullptr, (int)rows_cap, cv.at(c_counts), st)) != PGP_OK)
    return rc;
  int h_counts[5] = {0, 0, 0, 0, 0};
  if (roots) PGP_HIP(hipMemcpyAsync(roots, cv.at(c_roots), n * 4, hipMemcpyDeviceToHost, st));
  if (ids) PGP_HIP(hipMemcpyAsync(ids, cv.at(c_ids), n * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipMemcpyAsync(h_counts, cv.at(c_counts), 20, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  const size_t written = std::min((size_t)h_counts[0], rows_cap);   // rows beyond the kept count stay as the caller left them
  if (written) {
    PGP_HIP(hipMemcpyAsync(info, cv.at(c_info), written * sizeof(pgp_component_info), hipMemcpyDeviceToHost, st));
    PGP_HIP(hipStreamSynchronize(st));
  }
  std::memcpy(counts, h_counts, 20);
  return PGP_OK;
}

}  // extern "C"

// ---- PPF Hough voting (ppf_vote.hip) ----------------------------------------------------------------------------
extern "C" {

int pgp_ppf_default_options(pgp_ppf_options* opt) {
  if (!opt) {
    set_error("pgp_ppf_default_options: null");
    return PGP_EINVAL;
  }
  opt->ref_step = 5;
  opt->n_bins = 30;
  opt->peaks_per_ref = 1;
  opt->min_vote_fraction = 0.9f;
  opt->min_votes = 3;
  return PGP_OK;
}

int pgp_set_ppf_model(pgp_ctx* ctx, const float* xyz, const float* nrm, int n) {
  if (!ctx || n < 0 || (n > 0 && (!xyz || !nrm))) {
    set_error("pgp_set_ppf_model: bad argument (n = %d; positions and normals)", n);
    return PGP_EINVAL;
  }
  for (size_t i = 0; i < (size_t)n * 3; ++i)
    if (!std::isfinite(xyz[i]) || !std::isfinite(nrm[i])) {
      set_error("pgp_set_ppf_model: point %zu is not finite", i / 3);
      return PGP_EINVAL;
    }
  CtxGuard guard(ctx);
  PGP_HIP(hipDeviceSynchronize());   // a queued vote may still read the old model
  ctx->ppf_alpha_ready = false;
  ctx->ppf_model_n = -1;
  std::vector<float4> h((size_t)std::max(2 * n, 1));
  for (int i = 0; i < n; ++i) {
    h[i] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.f);
    h[(size_t)n + i] = make_float4(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], 0.f);
  }
  int rc = ctx->d_ppf_model.ensure(h.size() * sizeof(float4));
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(ctx->d_ppf_model.p, h.data(), h.size() * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  ctx->ppf_model_n = n;
  return ppf_model_angles(ctx);
}

int pgp_ppf_vote_device(pgp_ctx* ctx, const pgp_ppf_options* opt, float* d_T, int* d_votes, int* d_ref, int* d_cell,
                        int cap, int* d_n_out, void* stream) {
  if (!ctx || cap < 0 || !d_n_out || (cap > 0 && (!d_T || !d_votes))) {
    set_error("pgp_ppf_vote_device: bad argument");
    return PGP_EINVAL;
  }
  int rc = ppf_vote_check(ctx, opt, "pgp_ppf_vote_device");
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  rc = launch_ppf_vote(ctx, opt, nullptr, 0, nullptr, d_T, d_votes, d_ref, d_cell, cap, d_n_out, 0, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_ppf_vote(pgp_ctx* ctx, const pgp_ppf_options* opt, float* T, int* votes, int* ref, int* cell, int cap, int* n_out) {
  if (!ctx || cap < 0 || !n_out || (cap > 0 && (!T || !votes))) {
    set_error("pgp_ppf_vote: bad argument");
    return PGP_EINVAL;
  }
  int rc = ppf_vote_check(ctx, opt, "pgp_ppf_vote");
  if (rc != PGP_OK) return rc;
  *n_out = 0;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const int m = std::min(cap, ppf_slots(ctx, opt));   // no more hypotheses than slots
  const size_t b_T = ((size_t)m * 64 + 255) & ~(size_t)255, b_i = ((size_t)m * 4 + 255) & ~(size_t)255;
  if ((rc = ctx->d_ppf_io.ensure(b_T + 3 * b_i + 256)) != PGP_OK) return rc;
  unsigned char* base = ctx->d_ppf_io.as<unsigned char>();
  float* d_T = reinterpret_cast<float*>(base);
  int* d_v = reinterpret_cast<int*>(base + b_T);
  int* d_r = reinterpret_cast<int*>(base + b_T + b_i);
  int* d_c = reinterpret_cast<int*>(base + b_T + 2 * b_i);
  int* d_n = reinterpret_cast<int*>(base + b_T + 3 * b_i);
  if ((rc = launch_ppf_vote(ctx, opt, nullptr, 0, nullptr, d_T, d_v, d_r, d_c, m, d_n, 0, st)) != PGP_OK) return rc;
  int n = 0;
  PGP_HIP(hipMemcpyAsync(&n, d_n, 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  const int k = std::min(n, m);
  if (k > 0) {
    PGP_HIP(hipMemcpyAsync(T, d_T, (size_t)k * 64, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipMemcpyAsync(votes, d_v, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    if (ref) PGP_HIP(hipMemcpyAsync(ref, d_r, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    if (cell) PGP_HIP(hipMemcpyAsync(cell, d_c, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipStreamSynchronize(st));
  }
  *n_out = n;
  return PGP_OK;
}

int pgp_ppf_hypotheses(pgp_ctx* ctx, const pgp_ppf_options* opt, int mode, float gate_deg, float* T, float* scores,
                       int* votes, int cap, int* n_out, int* best_index, float* best_score, float* best_T) {
  if (!ctx || cap < 0 || !n_out || (cap > 0 && (!T || !scores)) || (mode != PGP_MODE_PLAIN && mode != PGP_MODE_WEIGHTED)) {
    set_error("pgp_ppf_hypotheses: bad argument");
    return PGP_EINVAL;
  }
  int rc = ppf_vote_check(ctx, opt, "pgp_ppf_hypotheses");
  if (rc != PGP_OK) return rc;
  *n_out = 0;
  if (best_index) *best_index = -1;
  if (best_score) *best_score = 0.f;
  CtxGuard guard(ctx);
  const int n_slots = ppf_slots(ctx, opt);
  if (n_slots == 0) return PGP_OK;
  if ((rc = reserve_impl(ctx, n_slots)) != PGP_OK) return rc;
  hipStream_t st = ctx->stream;
  // every slot is scored: the list, then NaN transforms (score 0) up to the slot count -- the host never needs the count
  // before the scoring launch, so the call synchronises once
  const size_t b_T = ((size_t)n_slots * 64 + 255) & ~(size_t)255, b_i = ((size_t)n_slots * 4 + 255) & ~(size_t)255;
  if ((rc = ctx->d_ppf_io.ensure(b_T + 2 * b_i + 256)) != PGP_OK) return rc;
  unsigned char* base = ctx->d_ppf_io.as<unsigned char>();
  float* d_T = reinterpret_cast<float*>(base);
  int* d_v = reinterpret_cast<int*>(base + b_T);
  float* d_s = reinterpret_cast<float*>(base + b_T + b_i);
  int* d_tail = reinterpret_cast<int*>(base + b_T + 2 * b_i);   // [0] count, [2..3] best {index, score bits}
  if ((rc = launch_ppf_vote(ctx, opt, nullptr, 0, nullptr, d_T, d_v, nullptr, nullptr, n_slots, d_tail, n_slots, st)) != PGP_OK)
    return rc;
  if ((rc = launch_score(ctx, d_T, n_slots, mode, gate_deg, d_s, nullptr, d_tail + 2, st)) != PGP_OK) return rc;
  const int m = std::min(cap, n_slots);
  std::vector<float> hT((size_t)m * 16), hs(m);
  std::vector<int> hv(m);
  int tail[4] = {0, 0, -1, 0};
  if (m > 0) {
    PGP_HIP(hipMemcpyAsync(hT.data(), d_T, (size_t)m * 64, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipMemcpyAsync(hs.data(), d_s, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipMemcpyAsync(hv.data(), d_v, (size_t)m * 4, hipMemcpyDeviceToHost, st));
  }
  PGP_HIP(hipMemcpyAsync(tail, d_tail, 16, hipMemcpyDeviceToHost, st));
  std::vector<float> bT(16);
  int b_idx = -1;
  PGP_HIP(hipStreamSynchronize(st));
  const int n = tail[0];
  b_idx = tail[2];
  if (b_idx >= n) b_idx = -1;   // (a pad scores 0 and is never the best; belt and braces)
  const int k = std::min(n, m);
  if (k > 0) {
    std::memcpy(T, hT.data(), (size_t)k * 64);
    std::memcpy(scores, hs.data(), (size_t)k * 4);
    if (votes) std::memcpy(votes, hv.data(), (size_t)k * 4);
  }
  if (b_idx >= 0 && best_T) {
    if (b_idx < m) std::memcpy(best_T, hT.data() + (size_t)b_idx * 16, 64);
    else PGP_HIP(hipMemcpy(best_T, d_T + (size_t)b_idx * 16, 64, hipMemcpyDeviceToHost));
  }
  *n_out = n;
  if (best_index) *best_index = b_idx;
  if (best_score) std::memcpy(best_score, &tail[3], 4);
  if (best_score && b_idx < 0) *best_score = 0.f;
  return PGP_OK;
}

int pgp_ppf_model_angles(pgp_ctx* ctx, float* alpha, long long n) {
  if (!ctx || n < 0 || (n > 0 && !alpha)) {
    set_error("pgp_ppf_model_angles: bad argument");
    return PGP_EINVAL;
  }
  if (!ctx->ppf_alpha_ready) {
    set_error("pgp_ppf_model_angles: no model angles (needs pgp_set_ppf_map with pairs and a covering pgp_set_ppf_model)");
    return PGP_ESTATE;
  }
  if (n != ctx->ppf_n_pairs) {
    set_error("pgp_ppf_model_angles: the table has %lld pairs, not %lld", ctx->ppf_n_pairs, n);
    return PGP_EINVAL;
  }
  if (n == 0) return PGP_OK;
  CtxGuard guard(ctx);
  PGP_HIP(hipMemcpyAsync(alpha, ctx->d_ppf_alpha.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  return PGP_OK;
}

int pgp_ppf_accumulator(pgp_ctx* ctx, const pgp_ppf_options* opt, const int* ref_ids, int k, int* acc) {
  if (!ctx || k < 0 || (k > 0 && (!ref_ids || !acc))) {
    set_error("pgp_ppf_accumulator: bad argument");
    return PGP_EINVAL;
  }
  int rc = ppf_vote_check(ctx, opt, "pgp_ppf_accumulator");
  if (rc != PGP_OK) return rc;
  for (int i = 0; i < k; ++i)
    if (ref_ids[i] < 0 || ref_ids[i] >= ctx->nP) {
      set_error("pgp_ppf_accumulator: reference %d names scene point %d of %d", i, ref_ids[i], ctx->nP);
      return PGP_EINVAL;
    }
  if (k == 0) return PGP_OK;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  const size_t cells = (size_t)ctx->ppf_model_n * opt->n_bins;
  const size_t b_r = ((size_t)k * 4 + 255) & ~(size_t)255, b_a = (std::max<size_t>(cells, 1) * k * 4 + 255) & ~(size_t)255;
  if ((rc = ctx->d_ppf_io.ensure(b_r + b_a + 256)) != PGP_OK) return rc;
  unsigned char* base = ctx->d_ppf_io.as<unsigned char>();
  int* d_ids = reinterpret_cast<int*>(base);
  int* d_acc = reinterpret_cast<int*>(base + b_r);
  int* d_n = reinterpret_cast<int*>(base + b_r + b_a);
  PGP_HIP(hipMemcpyAsync(d_ids, ref_ids, (size_t)k * 4, hipMemcpyHostToDevice, st));
  if ((rc = launch_ppf_vote(ctx, opt, d_ids, k, d_acc, nullptr, nullptr, nullptr, nullptr, 0, d_n, 0, st)) != PGP_OK) return rc;
  if (cells > 0) PGP_HIP(hipMemcpyAsync(acc, d_acc, cells * k * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

}  // extern "C"

// ---- physics settling of MCTS child states (physics.hip) --------------------------------------------------------
namespace {
size_t phys_al256(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

extern "C" {

int pgp_physics_default_options(pgp_physics_options* opt) {
  if (!opt) {
    set_error("pgp_physics_default_options: null");
    return PGP_EINVAL;
  }
  opt->dt = 1.f / 60.f;
  opt->steps = 60;
  opt->gravity[0] = 0.f;
  opt->gravity[1] = 0.f;
  opt->gravity[2] = -2.f;
  opt->linear_damping = 0.99f;
  opt->angular_damping = 0.99f;
  opt->friction = 1.f;
  opt->iterations = 10;
  opt->erp = 0.2f;
  return PGP_OK;
}

int pgp_convex_hull(const float* xyz, int n, int max_vertices, float* hull_xyz, int* n_vert, float* planes, int* n_planes) {
  if (!hull_xyz || !n_vert || !planes || !n_planes) {
    set_error("pgp_convex_hull: null output");
    return PGP_EINVAL;
  }
  std::vector<int> hv;
  std::vector<std::array<double, 4>> pl;
  const int rc = convex_hull_impl(xyz, n, max_vertices, hv, pl, "pgp_convex_hull");
  if (rc != PGP_OK) return rc;
  for (size_t i = 0; i < hv.size(); ++i)
    for (int c = 0; c < 3; ++c) hull_xyz[3 * i + c] = xyz[3 * (size_t)hv[i] + c];
  for (size_t f = 0; f < pl.size(); ++f)
    for (int c = 0; c < 4; ++c) planes[4 * f + c] = (float)pl[f][c];
  *n_vert = (int)hv.size();
  *n_planes = (int)pl.size();
  return PGP_OK;
}

int pgp_physics_add_shape(pgp_ctx* ctx, const float* xyz, int n, float margin, int max_vertices, int* shape_id) {
  if (!ctx || !shape_id || !(margin >= 0.f && margin <= 0.1f)) {
    set_error("pgp_physics_add_shape: bad argument");
    return PGP_EINVAL;
  }
  std::vector<int> hv;
  std::vector<std::array<double, 4>> pl;
  std::vector<int4> ed;
  std::vector<int> loop_off, loop_idx;
  int rc = convex_hull_impl(xyz, n, max_vertices, hv, pl, "pgp_physics_add_shape", &ed, &loop_off, &loop_idx);
  if (rc != PGP_OK) return rc;
  if ((int)ed.size() > PGP_PHYSICS_MAX_EDGES) {   // a closed hull of V vertices has at most 3 V - 6 edges
    set_error("pgp_physics_add_shape: %d hull edges (at most %d)", (int)ed.size(), PGP_PHYSICS_MAX_EDGES);
    return PGP_EINVAL;
  }
  // every edge is a side of two loops, every loop closes, and no loop outgrows the vertex cap (the settle kernel
  // sizes its polygon buffers by these)
  bool loops_ok = loop_off.size() == pl.size() + 1 && loop_idx.size() == 2 * ed.size();
  for (size_t f = 0; loops_ok && f < pl.size(); ++f) {
    const int len = loop_off[f + 1] - loop_off[f];
    loops_ok = len >= 3 && len <= PGP_PHYSICS_MAX_VERTICES;
  }
  if (!loops_ok) {
    set_error("pgp_physics_add_shape: the hull's face loops do not close (%d loop entries, %d edges)", (int)loop_idx.size(),
              (int)ed.size());
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  if ((rc = physics_arena_init(ctx)) != PGP_OK) return rc;
  std::vector<float4> v, p;
  for (int i : hv) v.push_back(make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.f));
  for (const auto& e : pl) p.push_back(make_float4((float)e[0], (float)e[1], (float)e[2], (float)e[3]));
  PGP_HIP(hipDeviceSynchronize());   // a queued settle may still read the arena that is about to grow
  arena_append(ctx, v, p, ed, loop_off, loop_idx, margin);
  if ((rc = arena_upload(ctx)) != PGP_OK) {
    arena_pop(ctx);
    return rc;
  }
  *shape_id = (int)ctx->phys_shapes.size() - 1;
  return PGP_OK;
}

int pgp_physics_shape_info(pgp_ctx* ctx, int shape_id, float* hull_xyz, int* n_vert, float* planes, int* n_planes,
                           float inertia[3], float* margin) {
  if (!ctx) {
    set_error("pgp_physics_shape_info: null context");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  int rc = physics_arena_init(ctx);
  if (rc != PGP_OK) return rc;
  if (shape_id < 0 || shape_id >= (int)ctx->phys_shapes.size()) {
    set_error("pgp_physics_shape_info: unknown shape %d", shape_id);
    return PGP_EINVAL;
  }
  PhysShape s;
  PGP_HIP(hipMemcpy(&s, ctx->d_phys_shapes.as<PhysShape>() + shape_id, sizeof(s), hipMemcpyDeviceToHost));
  std::vector<float4> v(s.n_vert), p(s.n_plane);
  PGP_HIP(hipMemcpy(v.data(), ctx->d_phys_verts.as<float4>() + s.vert_off, v.size() * sizeof(float4), hipMemcpyDeviceToHost));
  PGP_HIP(hipMemcpy(p.data(), ctx->d_phys_planes.as<float4>() + s.plane_off, p.size() * sizeof(float4), hipMemcpyDeviceToHost));
  if (n_vert) *n_vert = s.n_vert;
  if (n_planes) *n_planes = s.n_plane;
  if (hull_xyz)
    for (int i = 0; i < s.n_vert; ++i) {
      hull_xyz[3 * i] = v[i].x; hull_xyz[3 * i + 1] = v[i].y; hull_xyz[3 * i + 2] = v[i].z;
    }
  if (planes)
    for (int f = 0; f < s.n_plane; ++f) {
      planes[4 * f] = p[f].x; planes[4 * f + 1] = p[f].y; planes[4 * f + 2] = p[f].z; planes[4 * f + 3] = p[f].w;
    }
  if (inertia)
    for (int i = 0; i < 3; ++i) inertia[i] = s.inertia[i];
  if (margin) *margin = s.margin;
  return PGP_OK;
}

int pgp_physics_shape_edges(pgp_ctx* ctx, int shape_id, int* edges, int* n_edges) {
  if (!ctx) {
    set_error("pgp_physics_shape_edges: null context");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  int rc = physics_arena_init(ctx);
  if (rc != PGP_OK) return rc;
  if (shape_id < 0 || shape_id >= (int)ctx->phys_shapes.size()) {
    set_error("pgp_physics_shape_edges: unknown shape %d", shape_id);
    return PGP_EINVAL;
  }
  PhysEdgeSlice s;
  PGP_HIP(hipMemcpy(&s, ctx->d_phys_eslices.as<PhysEdgeSlice>() + shape_id, sizeof(s), hipMemcpyDeviceToHost));
  if (n_edges) *n_edges = s.n_edge;
  if (edges && s.n_edge > 0)
    PGP_HIP(hipMemcpy(edges, ctx->d_phys_edges.as<int4>() + s.edge_off, (size_t)s.n_edge * sizeof(int4), hipMemcpyDeviceToHost));
  return PGP_OK;
}

int pgp_physics_set_edge_contacts(pgp_ctx* ctx, int on, float reach) {
  if (!ctx || !(reach > 0.f) || !std::isfinite(reach)) {
    set_error("pgp_physics_set_edge_contacts: %s", !ctx ? "ctx is NULL" : "reach must be > 0 and finite");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  ctx->phys_edge_contacts = on != 0;
  ctx->phys_edge_reach = reach;
  return PGP_OK;
}

int pgp_physics_shape_faces(pgp_ctx* ctx, int shape_id, int* face_offsets, int* face_vertices, int* n_faces) {
  if (!ctx) {
    set_error("pgp_physics_shape_faces: null context");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  int rc = physics_arena_init(ctx);
  if (rc != PGP_OK) return rc;
  if (shape_id < 0 || shape_id >= (int)ctx->phys_shapes.size()) {
    set_error("pgp_physics_shape_faces: unknown shape %d", shape_id);
    return PGP_EINVAL;
  }
  PhysShape sh;
  PhysFaceSlice s;
  PGP_HIP(hipMemcpy(&sh, ctx->d_phys_shapes.as<PhysShape>() + shape_id, sizeof(sh), hipMemcpyDeviceToHost));
  PGP_HIP(hipMemcpy(&s, ctx->d_phys_fslices.as<PhysFaceSlice>() + shape_id, sizeof(s), hipMemcpyDeviceToHost));
  std::vector<int> off((size_t)sh.n_plane + 1);
  PGP_HIP(hipMemcpy(off.data(), ctx->d_phys_face_off.as<int>() + s.off_off, off.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (n_faces) *n_faces = sh.n_plane;
  if (face_offsets) std::copy(off.begin(), off.end(), face_offsets);
  if (face_vertices && off.back() > 0)
    PGP_HIP(hipMemcpy(face_vertices, ctx->d_phys_face_idx.as<int>() + s.idx_off, (size_t)off.back() * sizeof(int),
                      hipMemcpyDeviceToHost));
  return PGP_OK;
}

int pgp_physics_set_polyhedral_contacts(pgp_ctx* ctx, int on, float face_bias) {
  if (!ctx || !(face_bias >= 0.f) || !std::isfinite(face_bias)) {
    set_error("pgp_physics_set_polyhedral_contacts: %s", !ctx ? "ctx is NULL" : "face_bias must be >= 0 and finite");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  ctx->phys_poly_contacts = on != 0;
  ctx->phys_face_bias = face_bias;
  return PGP_OK;
}

int pgp_physics_settle(pgp_ctx* ctx, const pgp_physics_options* opt, int n_states, const int* dyn_shape, const float* T,
                       const int* static_offsets, const int* static_shape, const float* static_T,
                       const float table_params[12], const float cam_pose[16], float* T_out, pgp_physics_info* info) {
  const char* who = "pgp_physics_settle";
  if (!ctx || n_states < 0 || (n_states > 0 && (!dyn_shape || !T || !static_offsets || !T_out))) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  int rc = check_options(opt, who, PHYS_MAX_STEPS);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx);
  PhysParams P;
  if ((rc = make_params(ctx, opt, n_states, table_params, cam_pose, who, P)) != PGP_OK) return rc;
  if (n_states == 0) return PGP_OK;
  if ((rc = check_states(ctx, n_states, dyn_shape, T, static_offsets, static_shape, static_T, who)) != PGP_OK) return rc;
  const size_t n = (size_t)n_states, m = (size_t)static_offsets[n_states];
  const size_t b_dyn = phys_al256(n * 4), b_T = phys_al256(n * 64), b_off = phys_al256((n + 1) * 4), b_ss = phys_al256(std::max<size_t>(m, 1) * 4),
               b_sT = phys_al256(std::max<size_t>(m, 1) * 64), b_info = phys_al256(n * sizeof(pgp_physics_info));
  if ((rc = ctx->d_phys_io.ensure(b_dyn + 2 * b_T + b_off + b_ss + b_sT + b_info)) != PGP_OK) return rc;
  unsigned char* base = ctx->d_phys_io.as<unsigned char>();
  int* d_dyn = reinterpret_cast<int*>(base);
  float* d_T = reinterpret_cast<float*>(base + b_dyn);
  float* d_out = reinterpret_cast<float*>(base + b_dyn + b_T);
  int* d_off = reinterpret_cast<int*>(base + b_dyn + 2 * b_T);
  int* d_ss = reinterpret_cast<int*>(base + b_dyn + 2 * b_T + b_off);
  float* d_sT = reinterpret_cast<float*>(base + b_dyn + 2 * b_T + b_off + b_ss);
  pgp_physics_info* d_info = reinterpret_cast<pgp_physics_info*>(base + b_dyn + 2 * b_T + b_off + b_ss + b_sT);
  hipStream_t st = ctx->stream;
  PGP_HIP(hipMemcpyAsync(d_dyn, dyn_shape, n * 4, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_T, T, n * 64, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_off, static_offsets, (n + 1) * 4, hipMemcpyHostToDevice, st));
  if (m > 0) {
    PGP_HIP(hipMemcpyAsync(d_ss, static_shape, m * 4, hipMemcpyHostToDevice, st));
    PGP_HIP(hipMemcpyAsync(d_sT, static_T, m * 64, hipMemcpyHostToDevice, st));
  }
  if ((rc = launch_settle(ctx, P, d_dyn, d_T, d_off, d_ss, d_sT, d_out, d_info, nullptr, nullptr, nullptr, st)) != PGP_OK)
    return rc;
  PGP_HIP(hipMemcpyAsync(T_out, d_out, n * 64, hipMemcpyDeviceToHost, st));
  if (info) PGP_HIP(hipMemcpyAsync(info, d_info, n * sizeof(pgp_physics_info), hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

int pgp_physics_settle_device(pgp_ctx* ctx, const pgp_physics_options* opt, int n_states, const int* d_dyn_shape,
                              const float* d_T, const int* d_static_offsets, const int* d_static_shape,
                              const float* d_static_T, const float table_params[12], const float cam_pose[16],
                              float* d_T_out, pgp_physics_info* d_info, void* stream) {
  const char* who = "pgp_physics_settle_device";
  if (!ctx || n_states < 0 || (n_states > 0 && (!d_dyn_shape || !d_T || !d_static_offsets || !d_T_out))) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  int rc = check_options(opt, who, PHYS_MAX_STEPS);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx, false);
  PhysParams P;
  if ((rc = make_params(ctx, opt, n_states, table_params, cam_pose, who, P)) != PGP_OK) return rc;
  if (n_states == 0) return PGP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rc = launch_settle(ctx, P, d_dyn_shape, d_T, d_static_offsets, d_static_shape, d_static_T, d_T_out, d_info, nullptr,
                     nullptr, nullptr, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_physics_trace(pgp_ctx* ctx, const pgp_physics_options* opt, int dyn_shape, const float T[16], int n_static,
                      const int* static_shape, const float* static_T, const float table_params[12],
                      const float cam_pose[16], float* state, float* contacts, int* n_contacts) {
  const char* who = "pgp_physics_trace";
  if (!ctx || !T || n_static < 0 || n_static > PGP_PHYSICS_MAX_STATICS || !state || !contacts || !n_contacts) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  int rc = check_options(opt, who, PHYS_MAX_TRACE_STEPS);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx);
  PhysParams P;
  if ((rc = make_params(ctx, opt, 1, table_params, cam_pose, who, P)) != PGP_OK) return rc;
  const int off[2] = {0, n_static};
  if ((rc = check_states(ctx, 1, &dyn_shape, T, off, static_shape, static_T, who)) != PGP_OK) return rc;
  const size_t k = (size_t)opt->steps, m = (size_t)n_static;
  const size_t b_hdr = 256, b_T = 256, b_ss = phys_al256(std::max<size_t>(m, 1) * 4), b_sT = phys_al256(std::max<size_t>(m, 1) * 64),
               b_s = phys_al256(std::max<size_t>(k, 1) * PHYS_TRACE_STATE * 4),
               b_c = phys_al256(std::max<size_t>(k, 1) * PGP_PHYSICS_MAX_CONTACTS * PHYS_TRACE_CONTACT * 4), b_n = phys_al256(std::max<size_t>(k, 1) * 4);
  if ((rc = ctx->d_phys_io.ensure(b_hdr + 2 * b_T + b_ss + b_sT + b_s + b_c + b_n)) != PGP_OK) return rc;
  unsigned char* base = ctx->d_phys_io.as<unsigned char>();
  int* d_hdr = reinterpret_cast<int*>(base);   // [0] dyn, [1..2] offsets
  float* d_T = reinterpret_cast<float*>(base + b_hdr);
  float* d_out = reinterpret_cast<float*>(base + b_hdr + b_T);
  int* d_ss = reinterpret_cast<int*>(base + b_hdr + 2 * b_T);
  float* d_sT = reinterpret_cast<float*>(base + b_hdr + 2 * b_T + b_ss);
  float* d_s = reinterpret_cast<float*>(base + b_hdr + 2 * b_T + b_ss + b_sT);
  float* d_c = reinterpret_cast<float*>(base + b_hdr + 2 * b_T + b_ss + b_sT + b_s);
  int* d_n = reinterpret_cast<int*>(base + b_hdr + 2 * b_T + b_ss + b_sT + b_s + b_c);
  hipStream_t st = ctx->stream;
  const int hdr[3] = {dyn_shape, 0, n_static};
  PGP_HIP(hipMemcpyAsync(d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_T, T, 64, hipMemcpyHostToDevice, st));
  if (m > 0) {
    PGP_HIP(hipMemcpyAsync(d_ss, static_shape, m * 4, hipMemcpyHostToDevice, st));
    PGP_HIP(hipMemcpyAsync(d_sT, static_T, m * 64, hipMemcpyHostToDevice, st));
  }
  PGP_HIP(hipMemsetAsync(d_c, 0, b_c, st));
  if ((rc = launch_settle(ctx, P, d_hdr, d_T, d_hdr + 1, d_ss, d_sT, d_out, nullptr, d_s, d_c, d_n, st)) != PGP_OK) return rc;
  if (k > 0) {
    PGP_HIP(hipMemcpyAsync(state, d_s, k * PHYS_TRACE_STATE * 4, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipMemcpyAsync(contacts, d_c, k * PGP_PHYSICS_MAX_CONTACTS * PHYS_TRACE_CONTACT * 4, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipMemcpyAsync(n_contacts, d_n, k * 4, hipMemcpyDeviceToHost, st));
  }
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

}  // extern "C"

// ---- MCTS hypothesis selection (mcts.hip) -------------------------------------------------------------------------
extern "C" {

int pgp_mcts_default_options(pgp_mcts_options* opt) {
  if (!opt) {
    set_error("pgp_mcts_default_options: null");
    return PGP_EINVAL;
  }
  opt->max_expansions = 0;            // sum_{i=0..n_obj} 25^i (UCTSearch.cpp:290-293)
  opt->max_iterations = 2147483647;
  opt->max_seconds = 60.f;            // maxSearchTime (UCTSearch.cpp:10)
  opt->alpha = 5000.f;                // UCTState.cpp:10
  opt->explanation_threshold = 0.01f; // UCTState.cpp:8
  opt->rollout = PGP_MCTS_ROLLOUT_RANDOM;
  opt->seed = 0;
  opt->leaves_per_step = 1;
  opt->virtual_cost = 0.f;
  return pgp_physics_default_options(&opt->physics);
}

int pgp_mcts_search(pgp_ctx* ctx, const pgp_mcts_options* opt, const pgp_mcts_object* objs, int n_obj,
                    const float table_params[12], const float cam_pose[16], const pgp_camera* cam, const float* observed,
                    int* best_hyp, float* best_T, float* best_score, pgp_mcts_info* info, pgp_mcts_record* trace,
                    int trace_cap, int* n_trace) {
  if (!ctx) {
    set_error("pgp_mcts_search: null context");
    return PGP_EINVAL;
  }
  pgp_mcts_options def;
  if (!opt) {
    pgp_mcts_default_options(&def);
    opt = &def;
  }
  CtxGuard guard(ctx);
  return mcts_search_impl(ctx, opt, objs, n_obj, table_params, cam_pose, cam, observed, best_hyp, best_T, best_score,
                          info, trace, trace_cap, n_trace);
}

}  // extern "C"

// ---- trimmed ICP of MCTS states (tricp_states.hip) ------------------------------------------------------------------
extern "C" {

int pgp_tricp_default_options(pgp_tricp_options* opt) {
  if (!opt) {
    set_error("pgp_tricp_default_options: null");
    return PGP_EINVAL;
  }
  opt->trim_fraction = 0.5f;     // trimICPthreshold (UCTSearch.cpp:9)
  opt->removal_radius = 0.008f;  // pointRemovalThreshold (UCTState.cpp:9)
  opt->energy_ratio = 1.0f;      // UCTState.cpp:139
  opt->max_iterations = 100;
  return PGP_OK;
}

int pgp_tricp_set_objects(pgp_ctx* ctx, const pgp_tricp_object* objs, int n_obj) {
  const char* who = "pgp_tricp_set_objects";
  if (!ctx || n_obj < 0 || (n_obj > 0 && !objs)) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  size_t n_pts = 0;
  int max_seg = 0;
  for (int l = 0; l < n_obj; ++l) {
    const pgp_tricp_object& o = objs[l];
    if (o.n_model < 1 || o.n_model > PGP_TRICP_MAX_MODEL || !o.model_xyz) {
      set_error("%s: object %d has a model of %d points (1 .. %d expected)", who, l, o.n_model, PGP_TRICP_MAX_MODEL);
      return PGP_EINVAL;
    }
    if (o.n_segment < 0 || o.n_segment > PGP_TRICP_MAX_SEGMENT || (o.n_segment > 0 && !o.segment_xyz)) {
      set_error("%s: object %d has a segment of %d points (0 .. %d expected)", who, l, o.n_segment, PGP_TRICP_MAX_SEGMENT);
      return PGP_EINVAL;
    }
    n_pts += (size_t)o.n_model + (size_t)o.n_segment;
    max_seg = std::max(max_seg, o.n_segment);
  }
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  // nothing may still read the set that is replaced: a pgp_tricp_states_device launch queued on a caller's stream reads
  // the clouds through the resident table, so the whole device is drained, not the context's stream alone
  PGP_HIP(hipDeviceSynchronize());
  ctx->device_work_pending = false;
  ctx->tricp_n_obj = 0;
  ctx->tricp_max_seg = 0;
  if (n_obj == 0) {
    ctx->d_tricp_clouds.release();
    ctx->d_tricp_objs.release();
    return PGP_OK;
  }
  int rc;
  if ((rc = ctx->d_tricp_clouds.ensure(n_pts * sizeof(float4))) != PGP_OK) return rc;
  if ((rc = ctx->d_tricp_objs.ensure((size_t)n_obj * sizeof(TricpObject))) != PGP_OK) return rc;
  std::vector<float4> h(n_pts);
  std::vector<TricpObject> tab((size_t)n_obj);
  float4* d = ctx->d_tricp_clouds.as<float4>();
  size_t at = 0;
  for (int l = 0; l < n_obj; ++l) {
    const pgp_tricp_object& o = objs[l];
    tab[l].model = d + at;
    tab[l].n_model = o.n_model;
    for (int i = 0; i < o.n_model; ++i) h[at++] = make_float4(o.model_xyz[3 * i], o.model_xyz[3 * i + 1], o.model_xyz[3 * i + 2], 0.f);
    tab[l].seg = d + at;
    tab[l].n_seg = o.n_segment;
    for (int i = 0; i < o.n_segment; ++i)
      h[at++] = make_float4(o.segment_xyz[3 * i], o.segment_xyz[3 * i + 1], o.segment_xyz[3 * i + 2], 0.f);
  }
  PGP_HIP(hipMemcpyAsync(d, h.data(), n_pts * sizeof(float4), hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(ctx->d_tricp_objs.p, tab.data(), (size_t)n_obj * sizeof(TricpObject), hipMemcpyHostToDevice, st));
  PGP_HIP(hipStreamSynchronize(st));
  ctx->tricp_n_obj = n_obj;
  ctx->tricp_max_seg = max_seg;
  return PGP_OK;
}

int pgp_tricp_states(pgp_ctx* ctx, const pgp_tricp_options* opt, int n_states, const int* obj, float* T,
                     const int* static_offsets, const int* static_obj, const float* static_T, float* energy, int* iters,
                     int* n_kept) {
  const char* who = "pgp_tricp_states";
  if (!ctx || n_states < 0 || (n_states > 0 && (!obj || !T || !static_offsets))) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  pgp_tricp_options o;
  int rc = check_tricp_options(opt, who, o);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx);
  if (ctx->tricp_n_obj <= 0) {
    set_error("%s: no object set (pgp_tricp_set_objects)", who);
    return PGP_ESTATE;
  }
  if (n_states == 0) return PGP_OK;
  if (static_offsets[0] != 0) {
    set_error("%s: static_offsets[0] must be 0", who);
    return PGP_EINVAL;
  }
  for (int i = 0; i < n_states; ++i) {
    const int ns = static_offsets[i + 1] - static_offsets[i];
    if (obj[i] < 0 || obj[i] >= ctx->tricp_n_obj) {
      set_error("%s: state %d names object %d of %d", who, i, obj[i], ctx->tricp_n_obj);
      return PGP_EINVAL;
    }
    if (ns < 0 || ns > PGP_TRICP_MAX_STATICS) {
      set_error("%s: state %d has %d statics (0 .. %d expected)", who, i, ns, PGP_TRICP_MAX_STATICS);
      return PGP_EINVAL;
    }
    if (ns > 0 && (!static_obj || !static_T)) {
      set_error("%s: bad argument", who);
      return PGP_EINVAL;
    }
    for (int q = 0; q < 16; ++q)
      if (!std::isfinite(T[16 * (size_t)i + q])) {
        set_error("%s: state %d has a non-finite pose", who, i);
        return PGP_EINVAL;
      }
    for (int j = static_offsets[i]; j < static_offsets[i + 1]; ++j)
      if (static_obj[j] < 0 || static_obj[j] >= ctx->tricp_n_obj) {
        set_error("%s: state %d names static object %d of %d", who, i, static_obj[j], ctx->tricp_n_obj);
        return PGP_EINVAL;
      }
  }
  const size_t n = (size_t)n_states, m = (size_t)static_offsets[n_states];
  Carve cv;
  const auto p_obj = cv.add<int>(n, 256);
  const auto p_T = cv.add<float>(n * 16, 256);
  const auto p_off = cv.add<int>(n + 1, 256);
  const auto p_so = cv.add<int>(std::max<size_t>(m, 1), 256);
  const auto p_sT = cv.add<float>(std::max<size_t>(m, 1) * 16, 256);
  const auto p_e = cv.add<float>(n, 256);
  const auto p_it = cv.add<int>(n, 256);
  const auto p_nk = cv.add<int>(n, 256);
  if ((rc = cv.ensure(ctx->d_tricp_io)) != PGP_OK) return rc;
  hipStream_t st = ctx->stream;
  PGP_HIP(hipMemcpyAsync(cv.at(p_obj), obj, n * 4, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(cv.at(p_T), T, n * 64, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(cv.at(p_off), static_offsets, (n + 1) * 4, hipMemcpyHostToDevice, st));
  if (m > 0) {
    PGP_HIP(hipMemcpyAsync(cv.at(p_so), static_obj, m * 4, hipMemcpyHostToDevice, st));
    PGP_HIP(hipMemcpyAsync(cv.at(p_sT), static_T, m * 64, hipMemcpyHostToDevice, st));
  }
  if ((rc = launch_tricp_states(ctx, o, n_states, cv.at(p_obj), 0, cv.at(p_T), cv.at(p_off), cv.at(p_so), cv.at(p_sT),
                                cv.at(p_e), cv.at(p_it), cv.at(p_nk), st)) != PGP_OK)
    return rc;
  PGP_HIP(hipMemcpyAsync(T, cv.at(p_T), n * 64, hipMemcpyDeviceToHost, st));
  if (energy) PGP_HIP(hipMemcpyAsync(energy, cv.at(p_e), n * 4, hipMemcpyDeviceToHost, st));
  if (iters) PGP_HIP(hipMemcpyAsync(iters, cv.at(p_it), n * 4, hipMemcpyDeviceToHost, st));
  if (n_kept) PGP_HIP(hipMemcpyAsync(n_kept, cv.at(p_nk), n * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  return PGP_OK;
}

int pgp_tricp_states_device(pgp_ctx* ctx, const pgp_tricp_options* opt, int n_states, const int* d_obj, float* d_T,
                            const int* d_static_offsets, const int* d_static_obj, const float* d_static_T,
                            float* d_energy, int* d_iters, int* d_n_kept, void* stream) {
  const char* who = "pgp_tricp_states_device";
  // no static arrays at all: a batch without statics (the kernel then refuses a state whose range is not empty)
  if (!ctx || n_states < 0 || (n_states > 0 && (!d_obj || !d_T || !d_static_offsets || (!d_static_obj) != (!d_static_T)))) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  pgp_tricp_options o;
  int rc = check_tricp_options(opt, who, o);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx, false);
  if (ctx->tricp_n_obj <= 0) {
    set_error("%s: no object set (pgp_tricp_set_objects)", who);
    return PGP_ESTATE;
  }
  if (n_states == 0) return PGP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rc = launch_tricp_states(ctx, o, n_states, d_obj, 0, d_T, d_static_offsets, d_static_obj, d_static_T, d_energy, d_iters,
                           d_n_kept, st);
  note_device_work(ctx, st);
  return rc;
}

int pgp_mcts_set_tricp(pgp_ctx* ctx, int on, const pgp_tricp_options* opt) {
  const char* who = "pgp_mcts_set_tricp";
  if (!ctx) {
    set_error("%s: ctx is NULL", who);
    return PGP_EINVAL;
  }
  pgp_tricp_options o;
  const int rc = check_tricp_options(opt, who, o);
  if (rc != PGP_OK) return rc;   // nothing changes
  CtxGuard guard(ctx);
  ctx->mcts_tricp = on != 0;
  ctx->mcts_tricp_opt = o;
  return PGP_OK;
}

}  // extern "C"

// ---- the tail the matcher's one-call chains share ------------------------------------------------------------------------
namespace pgp {
namespace {
// the picked quads of a chain's resident batch into d_quads (launch_v4pcs_gather, launch_congruent_batch_gather)
using ChainGather = int (*)(pgp_ctx* ctx, const int* h_picks, int m, int4* d_quads, hipStream_t st);
// the caller's outputs of a chain call (pgp_v4pcs_hypotheses, pgp_super4pcs_hypotheses); nullable: pose and all from picks on
struct ChainOut {
  int* n_hyp;
  float* T;
  double* pose;
  int* status;
  float* scores;
  int *picks, *best_index;
  float *best_score, *best_T;
  double* best_pose;
};

// What follows a chain's join: at most max_per_base of every base's quads (counts[nb], the draw of pgp_sample_quads), their
// fits and plain scores on the device, the best.  `io` is the chain's own staging buffer, base_ids[4 nb] its bases.
int chain_tail(pgp_ctx* ctx, DevBuf& io, ChainGather gather, const int* base_ids, const int* counts, int nb, unsigned long long seed,
               int max_per_base, const float centroid_P[3], const float centroid_Q[3], const ChainOut& o) {
  hipStream_t st = ctx->stream;
  std::vector<int> pk((size_t)nb * (size_t)max_per_base * 2);
  int m = 0, rc;
  if ((rc = pgp_sample_quads(seed, counts, nb, max_per_base, pk.data(), &m)) != PGP_OK) return rc;
  if (m == 0) return PGP_OK;
  if ((rc = reserve_impl(ctx, m)) != PGP_OK) return rc;
  const size_t N = (size_t)m;
  Carve c;
  const auto p_pose = c.add<double>(16 * N, 16);
  const auto p_base = c.add<int4>(N, 16);
  const auto p_quad = c.add<int4>(N, 16);
  const auto p_T = c.add<float>(16 * N, 16);
  const auto p_rms = c.add<float>(N, 16);
  const auto p_status = c.add<int>(N, 16);
  const auto p_scores = c.add<float>(N, 16);
  if ((rc = c.ensure(io)) != PGP_OK) return rc;
  std::vector<int> hb(4 * N);
  pick_bases(pk.data(), N, base_ids, hb.data());
  PGP_HIP(hipMemcpyAsync(c.at(p_base), hb.data(), N * 16, hipMemcpyHostToDevice, st));
  if ((rc = gather(ctx, pk.data(), m, c.at(p_quad), st)) != PGP_OK) return rc;
  if ((rc = launch_rigid(ctx, reinterpret_cast<const int*>(c.at(p_base)), reinterpret_cast<const int*>(c.at(p_quad)), m, centroid_P,
                         centroid_Q, c.at(p_T), c.at(p_pose), c.at(p_status), c.at(p_rms), st)) != PGP_OK)
    return rc;
  // (the caller's transforms are the fits as pgp_rigid_from_congruent returns them; the scored copy has the failed ones masked)
  PGP_HIP(hipMemcpyAsync(o.T, c.at(p_T), N * 64, hipMemcpyDeviceToHost, st));
  hipLaunchKernelGGL(mask_failed_fits, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const int*)c.at(p_status), m, c.at(p_T));
  if ((rc = launch_score(ctx, c.at(p_T), m, PGP_MODE_PLAIN, 0.f, c.at(p_scores), nullptr, nullptr, st)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(o.scores, c.at(p_scores), N * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipMemcpyAsync(o.status, c.at(p_status), N * 4, hipMemcpyDeviceToHost, st));
  std::vector<double> h_pose;
  double* pose_dst = o.pose;
  if (!pose_dst && o.best_pose) {
    h_pose.resize(16 * N);
    pose_dst = h_pose.data();
  }
  if (pose_dst) PGP_HIP(hipMemcpyAsync(pose_dst, c.at(p_pose), N * 128, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  if ((rc = index_settled(ctx)) != PGP_OK) return rc;
  if (o.picks) std::memcpy(o.picks, pk.data(), N * 8);
  float bs = 0.f;
  const int bi = best_above_zero(o.scores, m, &bs);
  *o.n_hyp = m;
  if (o.best_index) *o.best_index = bi;
  if (o.best_score) *o.best_score = bs;
  if (bi >= 0 && o.best_T) std::memcpy(o.best_T, o.T + 16 * (size_t)bi, 64);
  if (bi >= 0 && o.best_pose) std::memcpy(o.best_pose, pose_dst + 16 * (size_t)bi, 128);
  return PGP_OK;
}
}  // namespace
}  // namespace pgp

// ---- tetrahedron-base mode, "V4PCS" (v4pcs.hip) ----------------------------------------------------------------------
namespace {
constexpr int kV4MaxTrials = 1 << 20;   // triangle / fourth-point draws per attempt
constexpr int kV4MaxAttempts = 1 << 20;

bool v4_dist_ok(const float* dist, int n_bases) {
  for (size_t k = 0; k < (size_t)n_bases * 6; ++k)
    if (!std::isfinite(dist[k])) return false;
  return true;
}
}  // namespace

extern "C" {

int pgp_select_tetrahedron_bases(pgp_ctx* ctx, unsigned long long seed, int n_attempts, int triangle_trials, int fourth_trials,
                                 float max_base_diameter, int* ids, float* dist, int* status) {
  if (!ctx || n_attempts < 0 || n_attempts > kV4MaxAttempts || triangle_trials < 0 || triangle_trials > kV4MaxTrials ||
      fourth_trials < 0 || fourth_trials > kV4MaxTrials || !(max_base_diameter > 0.f) ||
      (n_attempts > 0 && (!ids || !dist || !status))) {
    set_error("pgp_select_tetrahedron_bases: bad argument (attempts %d, trials %d / %d, diameter %g)", n_attempts, triangle_trials,
              fourth_trials, (double)max_base_diameter);
    return PGP_EINVAL;
  }
  if (n_attempts == 0) return PGP_OK;
  CtxGuard guard(ctx);
  return launch_tetrahedron_bases(ctx, seed, n_attempts, triangle_trials, fourth_trials, max_base_diameter, ids, dist, status,
                                  ctx->stream);
}

int pgp_find_congruent_v4pcs(pgp_ctx* ctx, const float dist[6], float eps, int* quads, int cap, long long* n_quads) {
  if (!ctx || !dist || !n_quads || cap < 0 || (cap > 0 && !quads) || !(eps >= 0.f) || !std::isfinite(eps) || !v4_dist_ok(dist, 1)) {
    set_error("pgp_find_congruent_v4pcs: bad argument");
    return PGP_EINVAL;
  }
  *n_quads = 0;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  int rc = ctx->d_v4_io.ensure((size_t)std::max(cap, 1) * 16);
  if (rc != PGP_OK) return rc;
  long long total = 0;
  if ((rc = launch_v4pcs_join(ctx, dist, 1, eps, cap, ctx->d_v4_io.as<int4>(), &total, st)) != PGP_OK) return rc;
  const long long n_copy = std::min<long long>(total, cap);
  if (n_copy > 0) {
    PGP_HIP(hipMemcpyAsync(quads, ctx->d_v4_io.p, (size_t)n_copy * 16, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipStreamSynchronize(st));
  }
  *n_quads = total;
  return PGP_OK;
}

int pgp_find_congruent_v4pcs_batch(pgp_ctx* ctx, const float* dist, int n_bases, float eps, int per_base_cap, long long* n_quads,
                                   int* n_stored) {
  if (!ctx || n_bases < 0 || n_bases > 65535 || per_base_cap < 1 || !(eps >= 0.f) || !std::isfinite(eps) ||
      (n_bases > 0 && (!dist || !v4_dist_ok(dist, n_bases)))) {
    set_error("pgp_find_congruent_v4pcs_batch: bad argument (%d bases, per_base_cap %d)", n_bases, per_base_cap);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_v4pcs_batch(ctx, dist, n_bases, eps, per_base_cap, n_quads, n_stored, ctx->stream);
}

int pgp_v4pcs_batch_quads(pgp_ctx* ctx, const int* picks, int m, int* quads) {
  if (!ctx || m < 0 || (m > 0 && (!picks || !quads))) {
    set_error("pgp_v4pcs_batch_quads: bad argument");
    return PGP_EINVAL;
  }
  if (m == 0) return PGP_OK;
  CtxGuard guard(ctx);
  int rc = ctx->d_v4_io.ensure((size_t)m * 16);
  if (rc != PGP_OK) return rc;
  if ((rc = launch_v4pcs_gather(ctx, picks, m, ctx->d_v4_io.as<int4>(), ctx->stream)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(quads, ctx->d_v4_io.p, (size_t)m * 16, hipMemcpyDeviceToHost, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  return PGP_OK;
}

int pgp_v4pcs_default_options(pgp_v4pcs_options* opt) {
  if (!opt) {
    set_error("pgp_v4pcs_default_options: null");
    return PGP_EINVAL;
  }
  opt->seed = 0;
  opt->n_bases = 100;           // base.cc:1837-1842
  opt->max_attempts = 200;
  opt->triangle_trials = 1000;  // kNumberOfDiameterTrials
  opt->fourth_trials = 100;
  opt->max_base_diameter = 0.f; // the caller's: the model's diameter or an estimate of it
  opt->eps = 0.005f;            // distance_factor * delta
  opt->max_per_base = 100;      // base.cc:1858-1874
  opt->per_base_cap = 4096;
  return PGP_OK;
}

int pgp_v4pcs_hypotheses(pgp_ctx* ctx, const pgp_v4pcs_options* opt, const float centroid_P[3], const float centroid_Q[3],
                         int* n_bases, int* base_ids, int* n_hyp, float* T, double* pose, int* status, float* scores, int* picks,
                         int* best_index, float* best_score, float* best_T, double* best_pose) {
  if (!ctx || !opt || !centroid_P || !centroid_Q || !n_hyp || !T || !status || !scores) {
    set_error("pgp_v4pcs_hypotheses: bad argument");
    return PGP_EINVAL;
  }
  if (opt->n_bases < 1 || opt->n_bases > 65535 || opt->max_attempts < 1 || opt->max_attempts > kV4MaxAttempts ||
      opt->triangle_trials < 0 || opt->triangle_trials > kV4MaxTrials || opt->fourth_trials < 0 || opt->fourth_trials > kV4MaxTrials ||
      !(opt->max_base_diameter > 0.f) || !(opt->eps >= 0.f) || !std::isfinite(opt->eps) || opt->max_per_base < 1 ||
      opt->max_per_base > kSampleMax || opt->per_base_cap < 1) {
    set_error("pgp_v4pcs_hypotheses: bad options (n_bases %d, max_attempts %d, trials %d / %d, diameter %g, eps %g, max_per_base %d of "
              "at most %d, per_base_cap %d)", opt->n_bases, opt->max_attempts, opt->triangle_trials, opt->fourth_trials,
              (double)opt->max_base_diameter, (double)opt->eps, opt->max_per_base, kSampleMax, opt->per_base_cap);
    return PGP_EINVAL;
  }
  *n_hyp = 0;
  if (n_bases) *n_bases = 0;
  if (best_index) *best_index = -1;
  if (best_score) *best_score = 0.f;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  // 1. attempts, the first n_bases successes kept in attempt order
  const size_t A = (size_t)opt->max_attempts;
  std::vector<int> a_ids(4 * A), a_status(A);
  std::vector<float> a_dist(6 * A);
  int rc = launch_tetrahedron_bases(ctx, opt->seed, opt->max_attempts, opt->triangle_trials, opt->fourth_trials, opt->max_base_diameter,
                                    a_ids.data(), a_dist.data(), a_status.data(), st);
  if (rc != PGP_OK) return rc;
  const std::vector<int> kept = first_successes(a_status.data(), opt->max_attempts, opt->n_bases);
  const int nb = (int)kept.size();
  std::vector<int> b_ids;
  std::vector<float> b_dist;
  for (const int a : kept) {
    b_ids.insert(b_ids.end(), a_ids.begin() + 4 * a, a_ids.begin() + 4 * a + 4);
    b_dist.insert(b_dist.end(), a_dist.begin() + 6 * a, a_dist.begin() + 6 * a + 6);
  }
  if (n_bases) *n_bases = nb;
  if (base_ids && nb > 0) std::memcpy(base_ids, b_ids.data(), (size_t)nb * 16);
  if (nb == 0) {   // no base: also no batch left behind that a pick could name
    ctx->v4_nb = 0;
    return PGP_OK;
  }
  // 2. the join: quads stay resident
  std::vector<int> stored((size_t)nb);
  if ((rc = launch_v4pcs_batch(ctx, b_dist.data(), nb, opt->eps, opt->per_base_cap, nullptr, stored.data(), st)) != PGP_OK) return rc;
  // 3. .. 5. at most max_per_base of every base's kept quads, their fits and plain scores, the best
  return chain_tail(ctx, ctx->d_v4_io, launch_v4pcs_gather, b_ids.data(), stored.data(), nb, opt->seed, opt->max_per_base, centroid_P,
                    centroid_Q, ChainOut{n_hyp, T, pose, status, scores, picks, best_index, best_score, best_T, best_pose});
}

}  // extern "C"

// ---- classic mode, "Super4PCS" (super4pcs.hip) ------------------------------------------------------------------------
extern "C" {

int pgp_select_wide_bases(pgp_ctx* ctx, unsigned long long seed, int n_attempts, int triangle_trials, float max_base_diameter,
                          int* ids, float* invariants, float* dist, int* status) {
  if (!ctx || n_attempts < 0 || n_attempts > kV4MaxAttempts || triangle_trials < 0 || triangle_trials > kV4MaxTrials ||
      !(max_base_diameter > 0.f) || !std::isfinite(max_base_diameter) ||
      (n_attempts > 0 && (!ids || !invariants || !dist || !status))) {
    set_error("pgp_select_wide_bases: bad argument (attempts %d, trials %d, diameter %g)", n_attempts, triangle_trials,
              (double)max_base_diameter);
    return PGP_EINVAL;
  }
  if (n_attempts == 0) return PGP_OK;
  CtxGuard guard(ctx);
  return launch_wide_bases(ctx, seed, n_attempts, triangle_trials, max_base_diameter, ids, invariants, dist, status, nullptr,
                           ctx->stream);
}

int pgp_extract_pairs_batch(pgp_ctx* ctx, const float* dist, int n_lists, float eps, int* n_pairs) {
  if (!ctx || n_lists < 0 || n_lists > 2 * 65535 || (n_lists > 0 && !dist) || !(eps >= 0.f) || !std::isfinite(eps)) {
    set_error("pgp_extract_pairs_batch: bad argument (%d lists)", n_lists);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_extract_pairs_batch(ctx, dist, n_lists, eps, n_pairs, ctx->stream);
}

int pgp_extract_pairs_batch_fetch(pgp_ctx* ctx, int list, int* pairs, int cap, int* n_pairs) {
  if (!ctx || !n_pairs || cap < 0 || (cap > 0 && !pairs)) {
    set_error("pgp_extract_pairs_batch_fetch: bad argument");
    return PGP_EINVAL;
  }
  *n_pairs = 0;
  CtxGuard guard(ctx);
  return extract_pairs_batch_fetch(ctx, list, pairs, cap, n_pairs, ctx->stream);
}

int pgp_find_congruent_batch_lists(pgp_ctx* ctx, const float* base_xyz, const float* invariants, const int* lists, int n_bases,
                                   float threshold, int* n_quads) {
  if (!ctx || n_bases < 0 || (n_bases > 0 && (!base_xyz || !invariants || !lists || !n_quads))) {
    set_error("pgp_find_congruent_batch_lists: bad argument");
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_find_congruent_batch_lists(ctx, base_xyz, invariants, lists, n_bases, threshold, n_quads, ctx->stream);
}

int pgp_super4pcs_default_options(pgp_super4pcs_options* opt) {
  if (!opt) {
    set_error("pgp_super4pcs_default_options: null");
    return PGP_EINVAL;
  }
  opt->seed = 0;
  opt->n_bases = 100;           // base.cc:1837-1842
  opt->max_attempts = 200;
  opt->triangle_trials = 1000;  // kNumberOfDiameterTrials
  opt->max_base_diameter = 0.f; // the caller's: the model's diameter or an estimate of it
  opt->eps = 0.005f;            // distance_factor * delta
  opt->max_per_base = 100;      // base.cc:1858-1874
  return PGP_OK;
}

}  // extern "C"

// the fields of a pgp_pair_gates that the calls refuse: a NaN, an infinity, a max_angle above 180
static bool pair_gates_ok(const pgp_pair_gates* g) {
  return !g || (std::isfinite(g->max_normal_difference) && std::isfinite(g->max_color_distance) &&
                std::isfinite(g->max_translation_distance) && std::isfinite(g->max_angle) && !(g->max_angle > 180.f));
}

static bool all_finite(const float* v, size_t count) {
  for (size_t k = 0; k < count; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// n x 3 host floats -> float4 {x, y, z, 0} in `buf`, synchronously
static int upload_xyz0(pgp_ctx* ctx, DevBuf& buf, const float* v, int n) {
  std::vector<float4> h((size_t)n);
  for (int i = 0; i < n; ++i) h[i] = make_float4(v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2], 0.f);
  const int rc = buf.ensure(h.size() * sizeof(float4));
  if (rc != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(buf.p, h.data(), h.size() * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  PGP_HIP(hipStreamSynchronize(ctx->stream));
  return PGP_OK;
}

// pgp_super4pcs_hypotheses and pgp_super4pcs_hypotheses_gated (gates nullable: none)
static int super4pcs_chain(pgp_ctx* ctx, const char* who, const pgp_super4pcs_options* opt, const pgp_pair_gates* gates,
                           const float centroid_P[3], const float centroid_Q[3], int* n_bases, int* base_ids, float* base_invariants,
                           int* n_hyp, float* T, double* pose, int* status, float* scores, int* picks, int* best_index,
                           float* best_score, float* best_T, double* best_pose) {
  if (!ctx || !opt || !centroid_P || !centroid_Q || !n_hyp || !T || !status || !scores) {
    set_error("%s: bad argument", who);
    return PGP_EINVAL;
  }
  if (opt->n_bases < 1 || opt->n_bases > 65535 || opt->max_attempts < 1 || opt->max_attempts > kV4MaxAttempts ||
      opt->triangle_trials < 0 || opt->triangle_trials > kV4MaxTrials || !(opt->max_base_diameter > 0.f) ||
      !std::isfinite(opt->max_base_diameter) || !(opt->eps >= 0.f) || !std::isfinite(opt->eps) || opt->max_per_base < 1 ||
      opt->max_per_base > kSampleMax) {
    set_error("%s: bad options (n_bases %d, max_attempts %d, trials %d, diameter %g, eps %g, max_per_base %d of "
              "at most %d)", who, opt->n_bases, opt->max_attempts, opt->triangle_trials, (double)opt->max_base_diameter, (double)opt->eps,
              opt->max_per_base, kSampleMax);
    return PGP_EINVAL;
  }
  if (!pair_gates_ok(gates)) {
    set_error("%s: bad gates (a NaN, an infinity or max_angle above 180)", who);
    return PGP_EINVAL;
  }
  *n_hyp = 0;
  if (n_bases) *n_bases = 0;
  if (best_index) *best_index = -1;
  if (best_score) *best_score = 0.f;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  // 1. attempts, the first n_bases successes kept in attempt order
  const size_t A = (size_t)opt->max_attempts;
  std::vector<int> a_ids(4 * A), a_status(A);
  std::vector<float> a_inv(2 * A), a_dist(2 * A), a_xyz(12 * A);
  int rc = launch_wide_bases(ctx, opt->seed, opt->max_attempts, opt->triangle_trials, opt->max_base_diameter, a_ids.data(), a_inv.data(),
                             a_dist.data(), a_status.data(), a_xyz.data(), st);
  if (rc != PGP_OK) return rc;
  const std::vector<int> kept = first_successes(a_status.data(), opt->max_attempts, opt->n_bases);
  const int nb = (int)kept.size();
  std::vector<int> b_ids, b_lists;
  std::vector<float> b_inv, b_dist, b_xyz;
  for (int b = 0; b < nb; ++b) {
    const int a = kept[b];
    b_ids.insert(b_ids.end(), a_ids.begin() + 4 * a, a_ids.begin() + 4 * a + 4);
    b_inv.insert(b_inv.end(), a_inv.begin() + 2 * a, a_inv.begin() + 2 * a + 2);
    b_dist.insert(b_dist.end(), a_dist.begin() + 2 * a, a_dist.begin() + 2 * a + 2);
    b_xyz.insert(b_xyz.end(), a_xyz.begin() + 12 * a, a_xyz.begin() + 12 * a + 12);
    b_lists.push_back(2 * b);       // pairs1: the list of |b0 b1|
    b_lists.push_back(2 * b + 1);   // pairs6: the list of |b2 b3|
  }
  if (n_bases) *n_bases = nb;
  if (base_ids && nb > 0) std::memcpy(base_ids, b_ids.data(), (size_t)nb * 16);
  if (base_invariants && nb > 0) std::memcpy(base_invariants, b_inv.data(), (size_t)nb * 8);
  if (nb == 0) return PGP_OK;
  // 2. the pair lists of the bases' 2 nb distances, resident; b_ids read as [2 nb][2] names the base edge of every list:
  //    (ids 0, 1) for pairs1, (ids 2, 3) for pairs6 (base.cc:1964-1968)
  if ((rc = launch_extract_pairs_batch_gated(ctx, b_dist.data(), b_ids.data(), 2 * nb, opt->eps, gates, nullptr, st)) != PGP_OK) return rc;
  // 3. the join, fed from those lists
  std::vector<int> nq((size_t)nb);
  if ((rc = launch_find_congruent_batch_lists(ctx, b_xyz.data(), b_inv.data(), b_lists.data(), nb, opt->eps, nq.data(), st)) != PGP_OK)
    return rc;
  // 4. .. 6. at most max_per_base of every base's quads, their fits and plain scores, the best
  const ChainGather gather = [](pgp_ctx* c, const int* h_picks, int m, int4* d_quads, hipStream_t s) {
    return launch_congruent_batch_gather(c, h_picks, m, d_quads, s);
  };
  return chain_tail(ctx, ctx->d_s4_io, gather, b_ids.data(), nq.data(), nb, opt->seed, opt->max_per_base, centroid_P, centroid_Q,
                    ChainOut{n_hyp, T, pose, status, scores, picks, best_index, best_score, best_T, best_pose});
}

extern "C" {

int pgp_super4pcs_hypotheses(pgp_ctx* ctx, const pgp_super4pcs_options* opt, const float centroid_P[3], const float centroid_Q[3],
                             int* n_bases, int* base_ids, float* base_invariants, int* n_hyp, float* T, double* pose, int* status,
                             float* scores, int* picks, int* best_index, float* best_score, float* best_T, double* best_pose) {
  return super4pcs_chain(ctx, "pgp_super4pcs_hypotheses", opt, nullptr, centroid_P, centroid_Q, n_bases, base_ids, base_invariants,
                         n_hyp, T, pose, status, scores, picks, best_index, best_score, best_T, best_pose);
}

int pgp_super4pcs_hypotheses_gated(pgp_ctx* ctx, const pgp_super4pcs_options* opt, const pgp_pair_gates* gates,
                                   const float centroid_P[3], const float centroid_Q[3], int* n_bases, int* base_ids,
                                   float* base_invariants, int* n_hyp, float* T, double* pose, int* status, float* scores, int* picks,
                                   int* best_index, float* best_score, float* best_T, double* best_pose) {
  return super4pcs_chain(ctx, "pgp_super4pcs_hypotheses_gated", opt, gates, centroid_P, centroid_Q, n_bases, base_ids,
                         base_invariants, n_hyp, T, pose, status, scores, picks, best_index, best_score, best_T, best_pose);
}

// ---- the classic mode's pair gates (super4pcs.hip pair_lists_gated) ---------------------------------------------------------
int pgp_pair_gates_default(pgp_pair_gates* gates) {
  if (!gates) {
    set_error("pgp_pair_gates_default: null");
    return PGP_EINVAL;
  }
  gates->max_normal_difference = -1.f;   // S4/super4pcs_test.cc:91-99: the fork's settings, all off
  gates->max_color_distance = -1.f;
  gates->max_translation_distance = -1.f;
  gates->max_angle = -1.f;
  gates->directed = 0;
  return PGP_OK;
}

int pgp_set_scene_colors(pgp_ctx* ctx, const float* rgb, int n) {
  if (!ctx || !rgb || n < 0) {
    set_error("pgp_set_scene_colors: bad argument (n=%d)", n);
    return PGP_EINVAL;
  }
  if (ctx->nP <= 0 || !ctx->d_P.p) {
    set_error("no scene: call pgp_set_scene first");
    return PGP_ESTATE;
  }
  if (n != ctx->nP || !all_finite(rgb, 3 * (size_t)n)) {
    set_error("pgp_set_scene_colors: %d colours for a scene of %d points, or a value that is not finite", n, ctx->nP);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  ctx->has_scene_colors = false;
  const int rc = upload_xyz0(ctx, ctx->d_Prgb, rgb, n);
  if (rc == PGP_OK) ctx->has_scene_colors = true;
  return rc;
}

int pgp_set_search_model_attributes(pgp_ctx* ctx, const float* nrm, const float* rgb, int n) {
  if (!ctx || n < 0) {
    set_error("pgp_set_search_model_attributes: bad argument (n=%d)", n);
    return PGP_EINVAL;
  }
  if (ctx->nQs <= 0 || !ctx->d_Qs.p) {
    set_error("no search model: call pgp_set_search_model first");
    return PGP_ESTATE;
  }
  if (n != ctx->nQs || (nrm && !all_finite(nrm, 3 * (size_t)n)) || (rgb && !all_finite(rgb, 3 * (size_t)n))) {
    set_error("pgp_set_search_model_attributes: %d attributes for a search model of %d points, or a value that is not finite", n,
              ctx->nQs);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  ctx->has_search_normals = ctx->has_search_colors = false;
  int rc;
  if (nrm) {
    if ((rc = upload_xyz0(ctx, ctx->d_Qs_nrm, nrm, n)) != PGP_OK) return rc;
    ctx->has_search_normals = true;
  }
  if (rgb) {
    if ((rc = upload_xyz0(ctx, ctx->d_Qs_rgb, rgb, n)) != PGP_OK) return rc;
    ctx->has_search_colors = true;
  }
  return PGP_OK;
}

int pgp_extract_pairs_batch_gated(pgp_ctx* ctx, const float* dist, const int* base_ids, int n_lists, float eps,
                                  const pgp_pair_gates* gates, int* n_pairs) {
  if (!ctx || n_lists < 0 || n_lists > 2 * 65535 || (n_lists > 0 && !dist) || !(eps >= 0.f) || !std::isfinite(eps) ||
      !pair_gates_ok(gates)) {
    set_error("pgp_extract_pairs_batch_gated: bad argument (%d lists; gates: a NaN, an infinity or max_angle above 180)", n_lists);
    return PGP_EINVAL;
  }
  CtxGuard guard(ctx);
  return launch_extract_pairs_batch_gated(ctx, dist, base_ids, n_lists, eps, gates, n_pairs, ctx->stream);
}

// ---- model preparation (model_prep.hip) ------------------------------------------------------------------------------------

static int check_sample_args(const char* who, const void* vertices, int n_vert, int stride, const void* triangles, int n_tri,
                             int n_samples, const void* xyz) {
  if (!vertices || !triangles || !xyz || n_vert < 1 || (stride != 3 && stride != 4) || n_tri < 1 || n_tri > PGP_SAMPLE_MESH_MAX_TRIANGLES ||
      n_samples < 1) {
    set_error("%s: bad argument (n_vert=%d, vertex_stride=%d, n_tri=%d of 1 .. %d, n_samples=%d)", who, n_vert, stride, n_tri,
              PGP_SAMPLE_MESH_MAX_TRIANGLES, n_samples);
    return PGP_EINVAL;
  }
  return PGP_OK;
}

// what the host forms check before anything is launched
static int check_mesh_host(const char* who, const float* vertices, int n_vert, int stride, const int* triangles, int n_tri) {
  for (size_t i = 0; i < (size_t)n_vert; ++i)
    for (int q = 0; q < 3; ++q)
      if (!std::isfinite(vertices[i * (size_t)stride + q])) {
        set_error("%s: vertex %zu is NaN or infinite", who, i);
        return PGP_EINVAL;
      }
  for (size_t i = 0; i < 3 * (size_t)n_tri; ++i)
    if (triangles[i] < 0 || triangles[i] >= n_vert) {
      set_error("%s: triangle %zu names vertex %d outside [0, %d)", who, i / 3, triangles[i], n_vert);
      return PGP_EINVAL;
    }
  return PGP_OK;
}

// the staged mesh and the dense sample of the host forms, one layout in ctx->d_prep_io
struct PrepStage {
  Carve cv;
  Carve::Piece<float> vert, xyz, nrm, rad, oxyz, onrm;
  Carve::Piece<int> tri, tid, order, otid;
  Carve::Piece<float4> xyz4;
};
static int prep_stage(pgp_ctx* ctx, PrepStage& s, int n_vert, int stride, int n_tri, int n_samples, int n_model, bool fps) {
  s.vert = s.cv.add<float>((size_t)n_vert * (size_t)stride, 256);
  s.tri = s.cv.add<int>(3 * (size_t)n_tri, 256);
  s.xyz = s.cv.add<float>(3 * (size_t)n_samples, 256);
  s.nrm = s.cv.add<float>(3 * (size_t)n_samples, 256);
  s.tid = s.cv.add<int>((size_t)n_samples, 256);
  if (fps) {
    s.xyz4 = s.cv.add<float4>((size_t)n_samples, 256);
    s.order = s.cv.add<int>((size_t)n_model, 256);
    s.rad = s.cv.add<float>((size_t)n_model, 256);
    s.oxyz = s.cv.add<float>(3 * (size_t)n_model, 256);
    s.onrm = s.cv.add<float>(3 * (size_t)n_model, 256);
    s.otid = s.cv.add<int>((size_t)n_model, 256);
  }
  return s.cv.ensure(ctx->d_prep_io);
}

int pgp_sample_mesh(pgp_ctx* ctx, const float* vertices, int n_vert, int vertex_stride, const int* triangles, int n_tri,
                    int n_samples, unsigned long long seed, float* xyz, float* nrm, int* tri) {
  if (!ctx) {
    set_error("pgp_sample_mesh: ctx is NULL");
    return PGP_EINVAL;
  }
  int rc = check_sample_args("pgp_sample_mesh", vertices, n_vert, vertex_stride, triangles, n_tri, n_samples, xyz);
  if (rc != PGP_OK || (rc = check_mesh_host("pgp_sample_mesh", vertices, n_vert, vertex_stride, triangles, n_tri)) != PGP_OK) return rc;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  PrepStage s;
  if ((rc = prep_stage(ctx, s, n_vert, vertex_stride, n_tri, n_samples, 0, false)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(s.cv.at(s.vert), vertices, s.vert.bytes(), hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(s.cv.at(s.tri), triangles, s.tri.bytes(), hipMemcpyHostToDevice, st));
  if ((rc = launch_sample_mesh(ctx, s.cv.at(s.vert), n_vert, vertex_stride, s.cv.at(s.tri), n_tri, n_samples, seed, s.cv.at(s.xyz),
                               nrm ? s.cv.at(s.nrm) : nullptr, tri ? s.cv.at(s.tid) : nullptr, nullptr, st)) != PGP_OK)
    return rc;
  HostOut out(ctx, st);
  if ((rc = out.to(xyz, s.cv.at(s.xyz), s.xyz.bytes())) != PGP_OK || (nrm && (rc = out.to(nrm, s.cv.at(s.nrm), s.nrm.bytes())) != PGP_OK) ||
      (tri && (rc = out.to(tri, s.cv.at(s.tid), s.tid.bytes())) != PGP_OK))
    return rc;
  return out.sync();
}

int pgp_sample_mesh_device(pgp_ctx* ctx, const float* d_vertices, int n_vert, int vertex_stride, const int* d_triangles, int n_tri,
                           int n_samples, unsigned long long seed, float* d_xyz, float* d_nrm, int* d_tri, void* stream) {
  if (!ctx) {
    set_error("pgp_sample_mesh_device: ctx is NULL");
    return PGP_EINVAL;
  }
  int rc = check_sample_args("pgp_sample_mesh_device", d_vertices, n_vert, vertex_stride, d_triangles, n_tri, n_samples, d_xyz);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx, false);
  rc = launch_sample_mesh(ctx, d_vertices, n_vert, vertex_stride, d_triangles, n_tri, n_samples, seed, d_xyz, d_nrm, d_tri, nullptr,
                          static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

static int check_fps_args(const char* who, const void* xyz, int n, int k, int start, const void* order) {
  if (!xyz || !order || n < 1 || k < 1 || k > n || start < -1 || start >= n) {
    set_error("%s: bad argument (n=%d, k=%d of 1 .. n, start=%d of -1 .. n - 1)", who, n, k, start);
    return PGP_EINVAL;
  }
  return PGP_OK;
}

int pgp_farthest_points(pgp_ctx* ctx, const float* xyz, int n, int k, int start, int* order, float* radius2) {
  if (!ctx) {
    set_error("pgp_farthest_points: ctx is NULL");
    return PGP_EINVAL;
  }
  int rc = check_fps_args("pgp_farthest_points", xyz, n, k, start, order);
  if (rc != PGP_OK) return rc;
  for (size_t i = 0; i < 3 * (size_t)n; ++i)
    if (!std::isfinite(xyz[i])) {
      set_error("pgp_farthest_points: point %zu is NaN or infinite", i / 3);
      return PGP_EINVAL;
    }
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  Carve cv;
  const auto c_in = cv.add<float>(3 * (size_t)n, 256);
  const auto c_p4 = cv.add<float4>((size_t)n, 256);
  const auto c_order = cv.add<int>((size_t)k, 256);
  const auto c_rad = cv.add<float>((size_t)k, 256);
  if ((rc = cv.ensure(ctx->d_prep_io)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(cv.at(c_in), xyz, c_in.bytes(), hipMemcpyHostToDevice, st));
  if ((rc = launch_pad4(cv.at(c_in), n, cv.at(c_p4), st)) != PGP_OK ||
      (rc = launch_farthest_points(ctx, cv.at(c_p4), n, k, start, cv.at(c_order), cv.at(c_rad), st)) != PGP_OK)
    return rc;
  HostOut out(ctx, st);
  if ((rc = out.to(order, cv.at(c_order), c_order.bytes())) != PGP_OK ||
      (radius2 && (rc = out.to(radius2, cv.at(c_rad), c_rad.bytes())) != PGP_OK))
    return rc;
  return out.sync();
}

int pgp_farthest_points_device(pgp_ctx* ctx, const float* d_xyz4, int n, int k, int start, int* d_order, float* d_radius2,
                               void* stream) {
  if (!ctx) {
    set_error("pgp_farthest_points_device: ctx is NULL");
    return PGP_EINVAL;
  }
  int rc = check_fps_args("pgp_farthest_points_device", d_xyz4, n, k, start, d_order);
  if (rc != PGP_OK) return rc;
  CtxGuard guard(ctx, false);
  rc = launch_farthest_points(ctx, reinterpret_cast<const float4*>(d_xyz4), n, k, start, d_order, d_radius2,
                              static_cast<hipStream_t>(stream));
  note_device_work(ctx, static_cast<hipStream_t>(stream));
  return rc;
}

int pgp_model_from_mesh(pgp_ctx* ctx, const float* vertices, int n_vert, int vertex_stride, const int* triangles, int n_tri,
                        int n_dense, int n_model, unsigned long long seed, float* xyz, float* nrm, int* tri, float* radius2) {
  if (!ctx) {
    set_error("pgp_model_from_mesh: ctx is NULL");
    return PGP_EINVAL;
  }
  int rc = check_sample_args("pgp_model_from_mesh", vertices, n_vert, vertex_stride, triangles, n_tri, n_dense, xyz);
  if (rc != PGP_OK) return rc;
  if (n_model < 1 || n_model > n_dense) {
    set_error("pgp_model_from_mesh: bad argument (n_model=%d of 1 .. n_dense=%d)", n_model, n_dense);
    return PGP_EINVAL;
  }
  if ((rc = check_mesh_host("pgp_model_from_mesh", vertices, n_vert, vertex_stride, triangles, n_tri)) != PGP_OK) return rc;
  CtxGuard guard(ctx);
  hipStream_t st = ctx->stream;
  PrepStage s;
  if ((rc = prep_stage(ctx, s, n_vert, vertex_stride, n_tri, n_dense, n_model, true)) != PGP_OK) return rc;
  PGP_HIP(hipMemcpyAsync(s.cv.at(s.vert), vertices, s.vert.bytes(), hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(s.cv.at(s.tri), triangles, s.tri.bytes(), hipMemcpyHostToDevice, st));
  if ((rc = launch_sample_mesh(ctx, s.cv.at(s.vert), n_vert, vertex_stride, s.cv.at(s.tri), n_tri, n_dense, seed, s.cv.at(s.xyz),
                               s.cv.at(s.nrm), s.cv.at(s.tid), s.cv.at(s.xyz4), st)) != PGP_OK ||
      (rc = launch_farthest_points(ctx, s.cv.at(s.xyz4), n_dense, n_model, -1, s.cv.at(s.order), s.cv.at(s.rad), st)) != PGP_OK ||
      (rc = launch_model_gather(s.cv.at(s.order), n_model, s.cv.at(s.xyz), s.cv.at(s.nrm), s.cv.at(s.tid), s.cv.at(s.oxyz),
                                s.cv.at(s.onrm), s.cv.at(s.otid), st)) != PGP_OK)
    return rc;
  HostOut out(ctx, st);
  if ((rc = out.to(xyz, s.cv.at(s.oxyz), s.oxyz.bytes())) != PGP_OK ||
      (nrm && (rc = out.to(nrm, s.cv.at(s.onrm), s.onrm.bytes())) != PGP_OK) ||
      (tri && (rc = out.to(tri, s.cv.at(s.otid), s.otid.bytes())) != PGP_OK) ||
      (radius2 && (rc = out.to(radius2, s.cv.at(s.rad), s.rad.bytes())) != PGP_OK))
    return rc;
  return out.sync();
}

}  // extern "C"
