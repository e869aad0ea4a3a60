// examples/model_from_mesh.cc -- a new object from nothing but its mesh, through the C ABI alone (include/pgp.h).  The node
// reads model_validation.ply, model_search.ply and PPFMap.txt per object, prepared offline (PPE/data_layer/Objects.cpp:
// 22-49); here all three come from the triangles:
//   1. pgp_model_from_mesh: 20 000 dense surface samples, the first 2 000 of their farthest-point order = the validation
//      cloud, whose first 400 rows are the search cloud (every prefix of the order is a farthest-point subset),
//   2. pgp_set_model, pgp_set_search_model and pgp_set_ppf_map_from_model install them,
//   3. a scene: the same mesh sampled again with another seed (20 000 points), moved by a known pose,
//   4. pgp_score_lcp, plain mode, delta = 5 mm, for the true pose and for one 3 cm off,
//   5. OK if the true pose scores >= 0.99 and the wrong one lower.  (About 25 scene points are expected in the 5 mm disc
//      around a model point, so a model point without a neighbour is an e^-25 event.)
// Usage:  model_from_mesh [mesh.obj]
//   mesh.obj: `v x y z` and `f a b c ...` lines are read (metres; a/b/c index forms and negative indices accepted,
//   polygons fan-triangulated), everything else is skipped.  Without it: a 0.16 x 0.10 x 0.06 m box with an off-centre
//   triangular prism on top.
#include <pgp.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define CHECK(x)                                                                 \
  do {                                                                           \
    int rc_ = (x);                                                               \
    if (rc_ != PGP_OK) {                                                         \
      std::printf("%s failed: %d (%s)\n", #x, rc_, pgp_last_error());           \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

namespace {

bool read_obj(const char* path, std::vector<float>* V, std::vector<int>* F) {
  std::ifstream f(path);
  if (!f.is_open()) return false;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream s(line);
    std::string tag;
    if (!(s >> tag)) continue;
    if (tag == "v") {
      float p[3];
      if (!(s >> p[0] >> p[1] >> p[2])) return false;
      V->insert(V->end(), p, p + 3);
    } else if (tag == "f") {
      std::vector<int> poly;
      std::string item;
      while (s >> item) {
        const long id = std::strtol(item.c_str(), nullptr, 10);   // stops at the first '/'
        const long n_vert = (long)(V->size() / 3);
        const long at = id > 0 ? id - 1 : n_vert + id;
        if (id == 0 || at < 0 || at >= n_vert) return false;
        poly.push_back((int)at);
      }
      if (poly.size() < 3) return false;
      for (size_t k = 1; k + 1 < poly.size(); ++k) {
        F->push_back(poly[0]);
        F->push_back(poly[k]);
        F->push_back(poly[k + 1]);
      }
    }
  }
  return !V->empty() && !F->empty();
}

// the box's 12 triangles and the prism's 7 (its base lies on the box), outward winding
void builtin_mesh(std::vector<float>* V, std::vector<int>* F) {
  const float hx = 0.08f, hy = 0.05f, hz = 0.03f;
  for (int i = 0; i < 8; ++i) {
    V->push_back(i & 1 ? hx : -hx);
    V->push_back(i & 2 ? hy : -hy);
    V->push_back(i & 4 ? hz : -hz);
  }
  const int box[12][3] = {{0, 2, 1}, {1, 2, 3}, {4, 5, 6}, {5, 7, 6}, {0, 1, 4}, {1, 5, 4},
                          {2, 6, 3}, {3, 6, 7}, {0, 4, 2}, {2, 4, 6}, {1, 3, 5}, {3, 7, 5}};
  for (int t = 0; t < 12; ++t) F->insert(F->end(), box[t], box[t] + 3);
  const float prism[6][3] = {{0.02f, -0.03f, hz}, {0.07f, -0.03f, hz}, {0.02f, 0.02f, hz},
                             {0.02f, -0.03f, 2 * hz}, {0.07f, -0.03f, 2 * hz}, {0.02f, 0.02f, 2 * hz}};
  for (int i = 0; i < 6; ++i) V->insert(V->end(), prism[i], prism[i] + 3);
  const int side[7][3] = {{3, 4, 5}, {0, 1, 4}, {0, 4, 3}, {1, 2, 5}, {1, 5, 4}, {2, 0, 3}, {2, 3, 5}};
  for (int t = 0; t < 7; ++t)
    for (int c = 0; c < 3; ++c) F->push_back(8 + side[t][c]);
}

// column-major [R | t]: a rotation of `angle` about the unit axis (x, y, z), then a translation
void make_pose(float angle, float x, float y, float z, const float t[3], float T[16]) {
  const float c = std::cos(angle), s = std::sin(angle);
  const float R[9] = {c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s,
                      y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s,
                      z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)};
  for (int k = 0; k < 16; ++k) T[k] = 0.f;
  for (int r = 0; r < 3; ++r)
    for (int col = 0; col < 3; ++col) T[r + 4 * col] = R[3 * r + col];
  for (int r = 0; r < 3; ++r) T[12 + r] = t[r];
  T[15] = 1.f;
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<float> V;
  std::vector<int> F;
  if (argc > 1) {
    if (!read_obj(argv[1], &V, &F)) {
      std::printf("cannot read a mesh from %s\n", argv[1]);
      return 1;
    }
  } else {
    builtin_mesh(&V, &F);
  }
  const int n_vert = (int)(V.size() / 3), n_tri = (int)(F.size() / 3);
  const int n_dense = 20000, n_model = 2000, n_search = 400, n_scene = 20000;
  const float delta = 0.005f;

  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  // 1. the validation cloud in farthest-point order; its first n_search rows are the search cloud
  std::vector<float> M((size_t)n_model * 3), Mn((size_t)n_model * 3), radius2(n_model);
  std::vector<int> Mt(n_model);
  CHECK(pgp_model_from_mesh(ctx, V.data(), n_vert, 3, F.data(), n_tri, n_dense, n_model, 1ull, M.data(), Mn.data(), Mt.data(),
                            radius2.data()));
  // 2. installed: validation model, search model and the search model's pair-feature table
  int n_keys = 0;
  long long n_pairs = 0;
  CHECK(pgp_set_model(ctx, M.data(), Mn.data(), n_model));
  CHECK(pgp_set_search_model(ctx, M.data(), n_search));
  CHECK(pgp_set_ppf_map_from_model(ctx, M.data(), Mn.data(), n_search, &n_keys, &n_pairs));
  // 3. a scene: other samples of the same surface, under a known pose
  std::vector<float> S((size_t)n_scene * 3), Sn((size_t)n_scene * 3), P((size_t)n_scene * 3), Pn((size_t)n_scene * 3),
      w(n_scene, 1.f);
  CHECK(pgp_sample_mesh(ctx, V.data(), n_vert, 3, F.data(), n_tri, n_scene, 2ull, S.data(), Sn.data(), nullptr));
  const float t_true[3] = {0.30f, -0.10f, 0.70f}, t_off[3] = {0.33f, -0.10f, 0.70f};
  float T[32];
  make_pose(0.4f, 0.6f, 0.0f, 0.8f, t_true, T);
  make_pose(0.4f, 0.6f, 0.0f, 0.8f, t_off, T + 16);
  for (int i = 0; i < n_scene; ++i)
    for (int r = 0; r < 3; ++r) {
      P[3 * i + r] = T[r] * S[3 * i] + T[4 + r] * S[3 * i + 1] + T[8 + r] * S[3 * i + 2] + T[12 + r];
      Pn[3 * i + r] = T[r] * Sn[3 * i] + T[4 + r] * Sn[3 * i + 1] + T[8 + r] * Sn[3 * i + 2];
    }
  CHECK(pgp_set_scene(ctx, P.data(), Pn.data(), w.data(), n_scene, delta));
  // 4. the true pose and one 3 cm off
  float scores[2] = {0.f, 0.f}, best_score = 0.f;
  int counts[2] = {0, 0}, best = -1;
  CHECK(pgp_score_lcp(ctx, T, 2, PGP_MODE_PLAIN, 30.f, scores, counts, &best, &best_score));
  CHECK(pgp_destroy(ctx));
  std::printf("%d vertices, %d triangles -> %d dense samples -> %d validation points (covering radius %.2f mm), "
              "%d search points (%.2f mm), %d keys, %lld pairs\n",
              n_vert, n_tri, n_dense, n_model, 1000.0 * std::sqrt((double)radius2[n_model - 1]), n_search,
              1000.0 * std::sqrt((double)radius2[n_search - 1]), n_keys, n_pairs);
  std::printf("plain LCP at %.0f mm: true pose %.4f (%d of %d), 3 cm off %.4f (%d)\n", 1000.0 * delta, scores[0], counts[0],
              n_model, scores[1], counts[1]);
  // 5.
  if (!(scores[0] >= 0.99f) || !(scores[1] < scores[0]) || best != 0) {
    std::printf("FAIL\n");
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
