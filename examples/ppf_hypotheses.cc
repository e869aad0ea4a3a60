// examples/ppf_hypotheses.cc -- the node's PPF_HOUGH generator through the C ABI alone (include/pgp.h):
//   PPFVoting::generate (PPE/hypothesis_generation/ObjectPoseCandidateSet.cpp:76-117) after its outlier filter and
//   normal flip: the object's PPFMap (Objects.cpp:31-49) -> pgp_set_ppf_map, pclModelSampled -> pgp_set_ppf_model,
//   pgp_ppf_hypotheses (votes, poses, LCP scores, bestHypothesis), then HypothesisSelection's greedy clustering on the
//   votes (pgp_cluster_poses).
// Usage:  ppf_hypotheses [seed]
// A synthetic object (a box with a cylinder on top, off centre: no symmetry) is sampled twice -- once as the model, once
// as the segment, moved by a known pose with 1 mm of noise -- so the program checks the best pose itself and ends "OK".
#include <pgp.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
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

// a point and its outward normal on the object's surface: box 0.16 x 0.10 x 0.06 centred at the origin, cylinder of
// radius 0.025, height 0.06 standing on its top face at (0.04, 0.01)
void sample_surface(std::mt19937& g, int n, std::vector<float>* xyz, std::vector<float>* nrm) {
  std::uniform_real_distribution<float> u(0.f, 1.f);
  const float bx = 0.16f, by = 0.10f, bz = 0.06f, r = 0.025f, h = 0.06f, cx = 0.04f, cy = 0.01f;
  const float faces[3] = {by * bz, bx * bz, bx * by};
  const float a_box = 2.f * (faces[0] + faces[1] + faces[2]), a_cyl = 2.f * 3.14159265f * r * h + 3.14159265f * r * r;
  for (int i = 0; i < n; ++i) {
    float p[3], q[3] = {0.f, 0.f, 0.f};
    if (u(g) * (a_box + a_cyl) < a_box) {
      float t = u(g) * a_box * 0.5f;
      const int ax = t < faces[0] ? 0 : (t < faces[0] + faces[1] ? 1 : 2);
      const float half[3] = {bx / 2, by / 2, bz / 2};
      const float sgn = u(g) < 0.5f ? -1.f : 1.f;
      for (int k = 0; k < 3; ++k) p[k] = (2.f * u(g) - 1.f) * half[k];
      p[ax] = sgn * half[ax];
      q[ax] = sgn;
    } else if (u(g) * a_cyl < 3.14159265f * r * r) {   // the cylinder's cap
      const float rad = r * std::sqrt(u(g)), th = 6.2831853f * u(g);
      p[0] = cx + rad * std::cos(th);
      p[1] = cy + rad * std::sin(th);
      p[2] = bz / 2 + h;
      q[2] = 1.f;
    } else {
      const float th = 6.2831853f * u(g);
      q[0] = std::cos(th);
      q[1] = std::sin(th);
      p[0] = cx + r * q[0];
      p[1] = cy + r * q[1];
      p[2] = bz / 2 + h * u(g);
    }
    for (int k = 0; k < 3; ++k) {
      xyz->push_back(p[k]);
      nrm->push_back(q[k]);
    }
  }
}

int approximate_bin(int val, int disc) {   // base.cc:150-160
  const int lower = val - (val % disc), upper = lower + disc;
  return (val - lower < upper - val) ? lower : upper;
}

// Match4PCSBase::computePPF of (i, j), u = p_i - p_j, as the node's PPFMap.txt holds it
std::array<int, 4> ppf(const float* p1, const float* n1, const float* p2, const float* n2) {
  const float u[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  auto angle = [](const float* a, const float* b) {
    const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float y = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), x = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    return approximate_bin(int(std::atan2(y, x) * 180 / M_PI), 10);
  };
  return {approximate_bin(int(std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) * 1000.f), 5), angle(n1, u), angle(n2, u),
          angle(n1, n2)};
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
  std::mt19937 g(seed);
  // the model (pclModelSampled: 500 points) and the validation model (2000), in the object frame
  std::vector<float> M, Mn, V, Vn;
  sample_surface(g, 500, &M, &Mn);
  sample_surface(g, 2000, &V, &Vn);
  // the segment: the object under a known pose (seeded axis, 20-160 degrees, 0.6 m away), its camera-facing half,
  // 1 mm of position noise; a pose error of pgp_pose_error is measured against it
  std::uniform_real_distribution<float> u(-1.f, 1.f);
  std::normal_distribution<float> noise(0.f, 0.001f);
  float ax[3] = {u(g), u(g), u(g)};
  const float al = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  for (float& a : ax) a /= al;
  const float ang = 0.35f + 2.4f * (0.5f + 0.5f * u(g)), c = std::cos(ang), s = std::sin(ang), C = 1.f - c;
  const float Rt[9] = {c + ax[0] * ax[0] * C,         ax[0] * ax[1] * C - ax[2] * s, ax[0] * ax[2] * C + ax[1] * s,
                       ax[1] * ax[0] * C + ax[2] * s, c + ax[1] * ax[1] * C,         ax[1] * ax[2] * C - ax[0] * s,
                       ax[2] * ax[0] * C - ax[1] * s, ax[2] * ax[1] * C + ax[0] * s, c + ax[2] * ax[2] * C};
  const float tt[3] = {0.02f * u(g), 0.02f * u(g), 0.6f};
  std::vector<float> S0, Sn0, P, Pn;
  sample_surface(g, 4000, &S0, &Sn0);
  for (size_t i = 0; i < S0.size() / 3; ++i) {
    float p[3], q[3];
    for (int r = 0; r < 3; ++r) {
      p[r] = Rt[3 * r] * S0[3 * i] + Rt[3 * r + 1] * S0[3 * i + 1] + Rt[3 * r + 2] * S0[3 * i + 2] + tt[r];
      q[r] = Rt[3 * r] * Sn0[3 * i] + Rt[3 * r + 1] * Sn0[3 * i + 1] + Rt[3 * r + 2] * Sn0[3 * i + 2];
    }
    if (q[0] * p[0] + q[1] * p[1] + q[2] * p[2] >= 0.f) continue;   // faces away from the camera at the origin
    for (int r = 0; r < 3; ++r) {
      P.push_back(p[r] + noise(g));
      Pn.push_back(q[r]);
    }
  }
  const int nP = (int)P.size() / 3, nM = (int)M.size() / 3, nV = (int)V.size() / 3;
  // the frames of Match4PCSBase::init: the segment minus its centroid, both models minus the search model's
  float cP[3], cQ[3];
  CHECK(pgp_center(P.data(), nP, M.data(), nM, V.data(), nV, cP, cQ));
  // the object's PPFMap over the search model, in the layout of PPFMap.txt
  std::map<std::array<int, 4>, std::vector<std::pair<int, int>>> table;
  for (int i = 0; i < nM; ++i)
    for (int j = 0; j < nM; ++j)
      if (i != j) table[ppf(&M[3 * i], &Mn[3 * i], &M[3 * j], &Mn[3 * j])].push_back(std::make_pair(i, j));
  std::vector<int> keys, counts, pairs;
  for (const auto& kv : table) {
    keys.insert(keys.end(), kv.first.begin(), kv.first.end());
    counts.push_back((int)kv.second.size());
    for (const auto& pr : kv.second) {
      pairs.push_back(pr.first);
      pairs.push_back(pr.second);
    }
  }
  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  std::vector<float> w(nP, 1.f);
  CHECK(pgp_set_scene(ctx, P.data(), Pn.data(), w.data(), nP, 0.005f));
  CHECK(pgp_set_model(ctx, V.data(), Vn.data(), nV));
  CHECK(pgp_set_search_model(ctx, M.data(), nM));
  CHECK(pgp_set_ppf_map(ctx, keys.data(), counts.data(), pairs.data(), (int)counts.size()));
  CHECK(pgp_set_ppf_model(ctx, M.data(), Mn.data(), nM));
  pgp_ppf_options opt;
  CHECK(pgp_ppf_default_options(&opt));
  const int cap = ((nP + opt.ref_step - 1) / opt.ref_step) * opt.peaks_per_ref;
  std::vector<float> T((size_t)cap * 16), scores(cap), best_T(16);
  std::vector<int> votes(cap);
  int n = 0, best = -1;
  float best_score = 0.f;
  CHECK(pgp_ppf_hypotheses(ctx, &opt, PGP_MODE_PLAIN, 30.f, T.data(), scores.data(), votes.data(), cap, &n, &best,
                           &best_score, best_T.data()));
  if (best < 0) {
    std::printf("no hypothesis scored above 0\n");
    return 1;
  }
  // greedy clustering on the votes (HypothesisSelection::greedyClustering with the vote count as the score)
  std::vector<float> fv(n);
  float top = 0.f;
  for (int i = 0; i < n; ++i) top = std::max(top, fv[i] = (float)votes[i]);
  std::vector<int> rep(n);
  int n_rep = 0;
  const float sym[3] = {0.f, 0.f, 0.f};
  CHECK(pgp_cluster_poses(ctx, T.data(), fv.data(), n, top, sym, nullptr, rep.data(), n, &n_rep, nullptr));
  // the true pose in the centred frames: x_c -> Rt (x_c + cQ) + tt - cP
  float gt[16] = {0};
  for (int r = 0; r < 3; ++r) {
    float t = tt[r] - cP[r];
    for (int k = 0; k < 3; ++k) {
      gt[4 * k + r] = Rt[3 * r + k];
      t += Rt[3 * r + k] * cQ[k];
    }
    gt[12 + r] = t;
  }
  gt[15] = 1.f;
  float rot = 0.f, trans = 0.f, rot_top = 0.f, trans_top = 0.f;
  CHECK(pgp_pose_error(ctx, best_T.data(), gt, 1, sym, &rot, &trans));
  CHECK(pgp_pose_error(ctx, &T[(size_t)rep[0] * 16], gt, 1, sym, &rot_top, &trans_top));
  std::printf("segment %d points, model %d, %zu keys: %d hypotheses, best %d (score %.4f, %d votes): %.2f deg, %.2f mm; "
              "%d clusters, the most voted %.2f deg, %.2f mm\n",
              nP, nM, counts.size(), n, best, best_score, votes[best], rot, 1000.f * trans, n_rep, rot_top, 1000.f * trans_top);
  CHECK(pgp_destroy(ctx));
  if (!(rot <= 5.f && trans <= 0.01f)) {
    std::printf("FAIL: the best pose is off\n");
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
