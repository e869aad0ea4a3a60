// examples/mcts_refine.cc -- the MCTS hypothesis selection with UCTState::performTrICP switched off and on
// (pgp_tricp_set_objects, pgp_mcts_set_tricp), through the C ABI alone.
// Two boxes touch along x on the table.  Each has two hypotheses within 5 mm and 5 degrees of the truth (yaw, x, y and a
// 2 mm lift).  The segment of a box is 120 points on each of three of its faces at the true pose (the R2
// low-discrepancy sequence), its model a 2 mm grid on all six faces; trim 0.9.  The observation is the truth rendered.
// The scene is tests/_tricp_scenes.py refine_example(), number for number; there the restatements show on the CPU that
// every refined leaf state ends nearer the truth than any unrefined one, in degrees and in millimetres, so the relation
// this program checks does not hinge on which state the render scores prefer.
// Prints, for the switch off and on, the best state, its render score and its error against the constructed truth (the
// two boxes' angles and distances added up); exits non-zero unless the refined error is below the unrefined one.
#include <pgp.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
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

const double kPi = 3.14159265358979323846;

void box(const double h[3], std::vector<float>& v) {
  v.clear();
  for (int i = 0; i < 8; ++i) {
    v.push_back((float)(i & 1 ? h[0] : -h[0]));
    v.push_back((float)(i & 2 ? h[1] : -h[1]));
    v.push_back((float)(i & 4 ? h[2] : -h[2]));
  }
}
const int kTris[36] = {0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5};

// the camera 0.8 m above the table top, looking straight down (its own inverse): camera = C . world, row-major 4x4
const double kCam[4][4] = {{1, 0, 0, 0}, {0, -1, 0, 0}, {0, 0, -1, 0.8}, {0, 0, 0, 1}};

// camera-frame pose (row-major double) of a world pose: yaw about +z, translation
void cam_pose(double yaw_deg, double x, double y, double z, double M[4][4]) {
  const double a = yaw_deg * kPi / 180.0, c = std::cos(a), s = std::sin(a);
  const double W[4][4] = {{c, -s, 0, x}, {s, c, 0, y}, {0, 0, 1, z}, {0, 0, 0, 1}};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc += kCam[i][k] * W[k][j];
      M[i][j] = acc;
    }
}
void colmajor(const double M[4][4], float* T) {
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 4; ++i) T[4 * j + i] = (float)M[i][j];
}

// a grid of about `step` on one face (axis, sign) of a box, appended to out (object frame)
void grid_face(const double h[3], int axis, double sign, double step, std::vector<float>& out) {
  const int b = (axis + 1) % 3, c = (axis + 2) % 3;
  const int nu = (int)std::floor(2 * h[b] / step + 0.5) + 1, nv = (int)std::floor(2 * h[c] / step + 0.5) + 1;
  for (int i = 0; i < nu; ++i)
    for (int j = 0; j < nv; ++j) {
      double q[3];
      q[axis] = sign * h[axis];
      q[b] = -h[b] + 2 * h[b] * i / (nu - 1);
      q[c] = -h[c] + 2 * h[c] * j / (nv - 1);
      for (int k = 0; k < 3; ++k) out.push_back((float)q[k]);
    }
}

// n points of the R2 sequence on one face, placed by M (row-major), appended to out (camera frame)
void r2_face(const double h[3], int axis, double sign, int n, const double M[4][4], std::vector<float>& out) {
  const int b = (axis + 1) % 3, c = (axis + 2) % 3;
  for (int i = 0; i < n; ++i) {
    const double u = std::fmod(0.5 + (i + 1) * 0.7548776662466927, 1.0), v = std::fmod(0.5 + (i + 1) * 0.5698402909980532, 1.0);
    double q[3];
    q[axis] = sign * h[axis];
    q[b] = (2 * u - 1) * h[b];
    q[c] = (2 * v - 1) * h[c];
    for (int r = 0; r < 3; ++r) out.push_back((float)(M[r][0] * q[0] + M[r][1] * q[1] + M[r][2] * q[2] + M[r][3]));
  }
}

// degrees and millimetres between a column-major pose and the truth (row-major double)
void pose_error(const float* T, const double M[4][4], double* deg, double* mm) {
  double tr = 0.0, d2 = 0.0;
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) tr += (double)T[4 * k + i] * M[i][k];   // trace(R Rt^T)
    const double d = (double)T[12 + i] - M[i][3];
    d2 += d * d;
  }
  double c = (tr - 1.0) / 2.0;
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
  *deg = std::acos(c) * 180.0 / kPi;
  *mm = std::sqrt(d2) * 1e3;
}

}  // namespace

int main() {
  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, 0));
  const float cam[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0.8f, 1};
  const float table[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.2f};
  pgp_camera K = {240, 320, 500.f, 500.f, 160.f, 120.f, 0.1f, 1.0f};
  const double half[2][3] = {{0.035, 0.03, 0.025}, {0.03, 0.03, 0.025}};
  const double centre[2][2] = {{0.0, 0.0}, {0.065, 0.0}};
  const int face_axis[2][3] = {{2, 0, 1}, {2, 0, 1}};
  const double face_sign[2][3] = {{1, -1, 1}, {1, 1, 1}};   // not the face the boxes share
  const double hyp[2][2][4] = {{{4.0, 0.003, -0.003, 0.002}, {-5.0, -0.003, 0.003, 0.002}},
                               {{-4.0, 0.002, 0.004, 0.002}, {5.0, -0.004, -0.002, 0.002}}};   // yaw, dx, dy, lift
  const int n_hyp = 2;

  std::vector<float> verts[2], model[2], segment[2], T[2], scores[2];
  double truth[2][4][4];
  float truth_T[2][16];
  int shape[2];
  for (int o = 0; o < 2; ++o) {
    box(half[o], verts[o]);
    CHECK(pgp_physics_add_shape(ctx, verts[o].data(), 8, 0.001f, 256, &shape[o]));
    cam_pose(0.0, centre[o][0], centre[o][1], half[o][2], truth[o]);
    colmajor(truth[o], truth_T[o]);
    for (int a = 0; a < 3; ++a)
      for (int s = 0; s < 2; ++s) grid_face(half[o], a, s ? 1.0 : -1.0, 0.002, model[o]);
    for (int f = 0; f < 3; ++f) r2_face(half[o], face_axis[o][f], face_sign[o][f], 120, truth[o], segment[o]);
    T[o].resize(16 * n_hyp);
    for (int h = 0; h < n_hyp; ++h) {
      double M[4][4];
      cam_pose(hyp[o][h][0], centre[o][0] + hyp[o][h][1], centre[o][1] + hyp[o][h][2], half[o][2] + hyp[o][h][3], M);
      colmajor(M, &T[o][16 * h]);
    }
    scores[o].assign(n_hyp, 0.5f);
  }
  // the observation: the truth rendered
  const size_t n_pix = (size_t)K.rows * K.cols;
  std::vector<float> img0(n_pix), observed(n_pix);
  CHECK(pgp_render_depth(ctx, verts[0].data(), 8, kTris, 12, truth_T[0], 1, &K, nullptr, img0.data()));
  CHECK(pgp_render_depth(ctx, verts[1].data(), 8, kTris, 12, truth_T[1], 1, &K, img0.data(), observed.data()));

  pgp_tricp_object clouds[2];
  pgp_mcts_object objs[2];
  for (int o = 0; o < 2; ++o) {
    clouds[o].model_xyz = model[o].data();
    clouds[o].n_model = (int)(model[o].size() / 3);
    clouds[o].segment_xyz = segment[o].data();
    clouds[o].n_segment = (int)(segment[o].size() / 3);
    objs[o].shape_id = shape[o];
    objs[o].vertices = verts[o].data();
    objs[o].vertex_stride = 3;
    objs[o].n_vert = 8;
    objs[o].triangles = kTris;
    objs[o].n_tri = 12;
    objs[o].n_hyp = n_hyp;
    objs[o].T = T[o].data();
    objs[o].scores = scores[o].data();
  }
  CHECK(pgp_tricp_set_objects(ctx, clouds, 2));
  pgp_tricp_options tr;
  CHECK(pgp_tricp_default_options(&tr));
  tr.trim_fraction = 0.9f;
  pgp_mcts_options opt;
  CHECK(pgp_mcts_default_options(&opt));
  opt.max_iterations = 64;   // the tree has 2 + 4 nodes: the search ends exhausted
  opt.leaves_per_step = 4;

  double err_deg[2], err_mm[2];
  for (int on = 0; on < 2; ++on) {
    CHECK(pgp_mcts_set_tricp(ctx, on, &tr));
    int best_hyp[2];
    float best_T[32], best_score = 0.f;
    pgp_mcts_info info;
    CHECK(pgp_mcts_search(ctx, &opt, objs, 2, table, cam, &K, observed.data(), best_hyp, best_T, &best_score, &info, nullptr,
                          0, nullptr));
    err_deg[on] = err_mm[on] = 0.0;
    for (int o = 0; o < 2; ++o) {
      double d, m;
      pose_error(best_T + 16 * o, truth[o], &d, &m);
      err_deg[on] += d;
      err_mm[on] += m;
    }
    std::printf("tricp %s: best (%d, %d) render score %.0f, %.3f deg %.3f mm from the truth (%lld descents, %.1f ms)\n",
                on ? "on " : "off", best_hyp[0], best_hyp[1], best_score, err_deg[on], err_mm[on], info.descents,
                info.elapsed_ms);
  }
  CHECK(pgp_mcts_set_tricp(ctx, 0, nullptr));
  CHECK(pgp_destroy(ctx));
  if (!(err_deg[1] < err_deg[0] && err_mm[1] < err_mm[0])) {
    std::printf("the refined best state is not nearer the truth than the unrefined one\n");
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
