// examples/mcts_search.cc -- the node's MCTS hypothesis selection (HypothesisSelection.cpp:241-265,
// UCTSearch::performSearch) through the C ABI alone: physics shapes and render meshes of two boxes, their hypothesis
// lists with LCP scores, one pgp_mcts_search call, the best state.
// The observation is the settled ground truth: box 1 stacked on box 0, both dropped from 1.5 cm, settled and rendered
// with pgp_physics_settle / pgp_render_depth.  Each box has 12 hypotheses: the lifted truth (not the top LCP score)
// and decoys shifted and turned.  The search must return the ground-truth ids at a cost no higher than the truth's.
// Prints OK or exits non-zero.
#include <pgp.h>

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

namespace {

void box(float hx, float hy, float hz, std::vector<float>& v) {
  v.clear();
  for (int i = 0; i < 8; ++i) {
    v.push_back(i & 1 ? hx : -hx);
    v.push_back(i & 2 ? hy : -hy);
    v.push_back(i & 4 ? hz : -hz);
  }
}
const int kTris[36] = {0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5};

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

}  // namespace

int main() {
  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, 0));
  // a camera 0.8 m above the table top (z = 0), looking straight down; tableParams: the box centre 0.2 m below
  const float cam[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8f, 1};
  const float cam_inv[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8f, 1};
  const float table[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.2f};
  pgp_camera K = {240, 320, 500.f, 500.f, 160.f, 120.f, 0.1f, 1.0f};
  const float half[2][3] = {{0.06f, 0.05f, 0.03f}, {0.035f, 0.03f, 0.025f}};
  const float truth[2][4] = {{10.f, 0.f, 0.f, 0.03f + 0.015f}, {-15.f, 0.005f, -0.004f, 0.06f + 0.025f + 0.015f}};
  const int n_hyp = 12, gt[2] = {7, 4};

  std::vector<float> verts[2];
  int shape[2];
  for (int o = 0; o < 2; ++o) {
    box(half[o][0], half[o][1], half[o][2], verts[o]);
    CHECK(pgp_physics_add_shape(ctx, verts[o].data(), 8, 0.001f, 256, &shape[o]));
  }
  // hypotheses: the lifted truth at gt[o] with the second-highest score, decoys around it
  std::mt19937 rng(5);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  std::vector<float> T[2], scores[2];
  for (int o = 0; o < 2; ++o) {
    T[o].resize(16 * n_hyp);
    scores[o].resize(n_hyp);
    for (int h = 0; h < n_hyp; ++h) {
      if (h == gt[o]) {
        cam_pose_of(cam_inv, truth[o][0], truth[o][1], truth[o][2], truth[o][3], &T[o][16 * h]);
        scores[o][h] = 0.85f;
      } else {
        const float a = 6.2831853f * U(rng), r = 0.05f + 0.07f * U(rng);
        cam_pose_of(cam_inv, truth[o][0] + 120.f * (U(rng) - 0.5f), truth[o][1] + r * std::cos(a),
                    truth[o][2] + r * std::sin(a), truth[o][3], &T[o][16 * h]);
        scores[o][h] = 0.1f + 0.7f * U(rng);
      }
    }
    scores[o][(gt[o] + 3) % n_hyp] = 0.95f;   // the top LCP score is a decoy
  }
  // the observation: the truth settled in objOrder (box 1 among box 0) and rendered
  pgp_physics_options phys;
  CHECK(pgp_physics_default_options(&phys));
  float settled[2][16];
  const int off0[2] = {0, 0}, off1[2] = {0, 1};
  CHECK(pgp_physics_settle(ctx, &phys, 1, &shape[0], &T[0][16 * gt[0]], off0, nullptr, nullptr, table, cam, settled[0],
                           nullptr));
  CHECK(pgp_physics_settle(ctx, &phys, 1, &shape[1], &T[1][16 * gt[1]], off1, &shape[0], settled[0], table, cam,
                           settled[1], nullptr));
  const size_t n_pix = (size_t)K.rows * K.cols;
  std::vector<float> img0(n_pix), observed(n_pix);
  CHECK(pgp_render_depth(ctx, verts[0].data(), 8, kTris, 12, settled[0], 1, &K, nullptr, img0.data()));
  CHECK(pgp_render_depth(ctx, verts[1].data(), 8, kTris, 12, settled[1], 1, &K, img0.data(), observed.data()));
  float truth_cost = 0.f;
  CHECK(pgp_depth_cost(ctx, observed.data(), observed.data(), 1, K.rows, K.cols, 0.01f, &truth_cost, nullptr));

  // the search: hypothesisSet, tableParams, camPose and depthImage of MCTSSelection::selectBestPoses
  pgp_mcts_object objs[2];
  for (int o = 0; o < 2; ++o)
    objs[o] = {shape[o], verts[o].data(), 3, 8, kTris, 12, n_hyp, T[o].data(), scores[o].data()};
  pgp_mcts_options opt;
  CHECK(pgp_mcts_default_options(&opt));
  opt.alpha = 500.f;
  opt.max_iterations = 2000;
  opt.leaves_per_step = 32;
  int best_hyp[2];
  float best_T[32], best_score = 0.f;
  pgp_mcts_info info;
  CHECK(pgp_mcts_search(ctx, &opt, objs, 2, table, cam, &K, observed.data(), best_hyp, best_T, &best_score, &info,
                        nullptr, 0, nullptr));
  float err = 0.f;
  for (int o = 0; o < 2; ++o)
    for (int k = 12; k < 15; ++k) err += (best_T[16 * o + k] - settled[o][k]) * (best_T[16 * o + k] - settled[o][k]);
  err = std::sqrt(err);
  std::printf("%lld descents in %lld steps, %lld expansions, %lld settled states, stop %d, %.1f ms: best (%d, %d) cost "
              "%.0f (truth (%d, %d) cost %.0f), %.3f mm from the settled truth\n",
              info.descents, info.steps, info.expansions, info.settle_evaluations, info.stop_reason, info.elapsed_ms,
              best_hyp[0], best_hyp[1], best_score, gt[0], gt[1], truth_cost, err * 1e3f);
  int bad = 0;
  if (best_hyp[0] != gt[0] || best_hyp[1] != gt[1]) bad = 1, std::printf("the search missed the ground truth\n");
  if (!(best_score <= truth_cost)) bad = 1, std::printf("the best cost exceeds the truth's\n");
  if (err > 1e-6f) bad = 1, std::printf("the best state's poses are not the settled truth\n");
  CHECK(pgp_destroy(ctx));
  if (bad) return 1;
  std::printf("OK\n");
  return 0;
}
