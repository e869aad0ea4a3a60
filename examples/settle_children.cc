// examples/settle_children.cc -- expands 64 children of one MCTS state through the C ABI alone:
// UCTState::correctPhysics -> UCTState::render -> UCTState::computeCost (UCTSearch.cpp:99,158,226) for all children
// at once, on one stream with one synchronisation:
//   pgp_physics_settle_device -> pgp_render_depth_device (under the parent's image) -> pgp_depth_cost_device.
// The scene: a table, one object placed earlier (static) and the new object, whose true pose rests on the table.
// One child holds the true pose lifted 2.5 cm above the table; the others are shifted or turned.  Unsettled, every
// child explains the observation badly; settled, the lifted child lands on the true pose and must win the cost.
// Prints OK or exits non-zero.
#include <pgp.h>
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CHECK(x)                                                                          \
  do {                                                                                    \
    int rc_ = (x);                                                                        \
    if (rc_ != 0) {                                                                       \
      std::fprintf(stderr, "%s failed: %d %s\n", #x, rc_, pgp_last_error());              \
      std::exit(1);                                                                       \
    }                                                                                     \
  } while (0)
#define HCHECK(x)                                                                         \
  do {                                                                                    \
    if ((x) != hipSuccess) {                                                              \
      std::fprintf(stderr, "%s failed\n", #x);                                            \
      std::exit(1);                                                                       \
    }                                                                                     \
  } while (0)

namespace {

const float HX = 0.03f, HY = 0.02f, HZ = 0.015f;   // the object: a 6 x 4 x 3 cm box

void box_mesh(std::vector<float>& v, std::vector<int>& tri) {
  for (int i = 0; i < 8; ++i) {
    v.push_back(i & 1 ? HX : -HX);
    v.push_back(i & 2 ? HY : -HY);
    v.push_back(i & 4 ? HZ : -HZ);
  }
  tri = {0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5};
}

// world pose (yaw about +z, translation) -> column-major camera-frame pose under cam_inv
void cam_pose_of(const float cam_inv[16], float yaw_deg, float x, float y, float z, float* T) {
  const float a = yaw_deg * 3.14159265f / 180.f, c = std::cos(a), s = std::sin(a);
  const float W[16] = {c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, x, y, z, 1};
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 4; ++i) {
      float acc = 0.f;
      for (int k = 0; k < 4; ++k) acc += cam_inv[k * 4 + i] * W[j * 4 + k];
      T[j * 4 + i] = acc;
    }
}

template <class T> T* upload(const std::vector<T>& h) {
  void* d = nullptr;
  HCHECK(hipMalloc(&d, h.size() * sizeof(T)));
  HCHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<T*>(d);
}

}  // namespace

int main() {
  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  std::vector<float> verts;
  std::vector<int> tris;
  box_mesh(verts, tris);
  int obj = -1;
  CHECK(pgp_physics_add_shape(ctx, verts.data(), 8, 0.001f, 256, &obj));

  // a camera 0.8 m above the table top (z = 0), looking straight down; tableParams: the box centre 0.2 m below
  const float cam[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8f, 1};
  const float cam_inv[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8f, 1};
  const float table[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.2f};
  pgp_camera K = {240, 320, 500.f, 500.f, 160.f, 120.f, 0.1f, 1.0f};
  const int npx = K.rows * K.cols;

  // the parent state: the earlier object, resting; the truth: the new object resting at (0.03, 0.01) turned 20 deg
  const float rest_z = HZ + 0.001f;   // resting height: the margin above the table
  float T_static[16], T_true[16];
  cam_pose_of(cam_inv, -10.f, -0.07f, -0.01f, rest_z, T_static);
  cam_pose_of(cam_inv, 20.f, 0.03f, 0.01f, rest_z, T_true);
  std::vector<float> parent(npx), observed(npx);
  CHECK(pgp_render_depth(ctx, verts.data(), 8, tris.data(), 12, T_static, 1, &K, nullptr, parent.data()));
  CHECK(pgp_render_depth(ctx, verts.data(), 8, tris.data(), 12, T_true, 1, &K, parent.data(), observed.data()));

  // 64 children: child 37 is the truth lifted by 2.5 cm, the others shifted by 1-4 cm and turned, at 0-3 cm
  const int n = 64, winner = 37;
  std::mt19937 rng(5);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  std::vector<float> T(16 * n), sT(16 * n);
  std::vector<int> dyn(n, obj), off(n + 1), ss(n, obj);
  for (int i = 0; i < n; ++i) {
    off[i] = i;
    for (int k = 0; k < 16; ++k) sT[16 * i + k] = T_static[k];
    if (i == winner) {
      cam_pose_of(cam_inv, 20.f, 0.03f, 0.01f, rest_z + 0.025f, &T[16 * i]);
      continue;
    }
    const float r = 0.01f + 0.03f * U(rng), a = 6.2831853f * U(rng);
    cam_pose_of(cam_inv, 20.f + 60.f * (U(rng) - 0.5f), 0.03f + r * std::cos(a), 0.01f + r * std::sin(a),
                rest_z + 0.03f * U(rng), &T[16 * i]);
  }
  off[n] = n;

  int* d_dyn = upload(dyn);
  float* d_T = upload(T);
  int* d_off = upload(off);
  int* d_ss = upload(ss);
  float* d_sT = upload(sT);
  float* d_verts = upload(verts);
  int* d_tris = upload(tris);
  float* d_parent = upload(parent);
  float* d_obs = upload(observed);
  float *d_depth = nullptr, *d_scores = nullptr;
  int* d_counts = nullptr;
  pgp_physics_info* d_info = nullptr;
  HCHECK(hipMalloc((void**)&d_depth, sizeof(float) * npx * n));
  HCHECK(hipMalloc((void**)&d_scores, sizeof(float) * n));
  HCHECK(hipMalloc((void**)&d_counts, sizeof(int) * 3 * n));
  HCHECK(hipMalloc((void**)&d_info, sizeof(pgp_physics_info) * n));
  hipStream_t st;
  HCHECK(hipStreamCreate(&st));

  // the children without physics, for comparison
  std::vector<float> unsettled(n);
  CHECK(pgp_render_depth_device(ctx, d_verts, 3, 8, d_tris, 12, d_T, n, &K, d_parent, 0, d_depth, st));
  CHECK(pgp_depth_cost_device(ctx, d_obs, d_depth, n, K.rows, K.cols, 0.01f, d_counts, d_scores, st));
  HCHECK(hipMemcpyAsync(unsettled.data(), d_scores, sizeof(float) * n, hipMemcpyDeviceToHost, st));
  HCHECK(hipStreamSynchronize(st));

  // the expansion: settle in place, render under the parent, cost -- one stream, one synchronisation
  pgp_physics_options opt;
  CHECK(pgp_physics_default_options(&opt));
  std::vector<float> scores(n), T_out(16 * n);
  std::vector<pgp_physics_info> info(n);
  CHECK(pgp_physics_settle_device(ctx, &opt, n, d_dyn, d_T, d_off, d_ss, d_sT, table, cam, d_T, d_info, st));
  CHECK(pgp_render_depth_device(ctx, d_verts, 3, 8, d_tris, 12, d_T, n, &K, d_parent, 0, d_depth, st));
  CHECK(pgp_depth_cost_device(ctx, d_obs, d_depth, n, K.rows, K.cols, 0.01f, d_counts, d_scores, st));
  HCHECK(hipMemcpyAsync(scores.data(), d_scores, sizeof(float) * n, hipMemcpyDeviceToHost, st));
  HCHECK(hipMemcpyAsync(T_out.data(), d_T, sizeof(float) * 16 * n, hipMemcpyDeviceToHost, st));
  HCHECK(hipMemcpyAsync(info.data(), d_info, sizeof(pgp_physics_info) * n, hipMemcpyDeviceToHost, st));
  HCHECK(hipStreamSynchronize(st));

  int best = 0;
  for (int i = 1; i < n; ++i)
    if (scores[i] < scores[best]) best = i;
  float err = 0.f;
  for (int k = 12; k < 15; ++k) err += (T_out[16 * winner + k] - T_true[k]) * (T_out[16 * winner + k] - T_true[k]);
  err = std::sqrt(err);
  std::printf("unsettled: child %d cost %.0f; settled: best child %d cost %.0f (child %d: %.0f, %d contacts, "
              "%.2f mm from the truth)\n",
              winner, unsettled[winner], best, scores[best], winner, scores[winner], info[winner].n_contacts, err * 1e3f);
  int bad = 0;
  if (best != winner) bad = 1, std::printf("the lifted true child does not win\n");
  if (err > 0.002f) bad = 1, std::printf("the lifted true child did not settle onto the truth\n");
  if (!(scores[winner] < unsettled[winner])) bad = 1, std::printf("settling did not lower the cost\n");
  for (void* p : {(void*)d_dyn, (void*)d_T, (void*)d_off, (void*)d_ss, (void*)d_sT, (void*)d_verts, (void*)d_tris,
                  (void*)d_parent, (void*)d_obs, (void*)d_depth, (void*)d_scores, (void*)d_counts, (void*)d_info})
    HCHECK(hipFree(p));
  HCHECK(hipStreamDestroy(st));
  CHECK(pgp_destroy(ctx));
  if (bad) return 1;
  std::printf("OK\n");
  return 0;
}
