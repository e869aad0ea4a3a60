// examples/match_oriented.cc -- two ORIENTED clouds in, a pose out, through the C ABI alone (include/pgp.h):
//   the matcher's classic mode with Match4PCSOptions::max_normal_difference = 20 degrees (pairCreationFunctor.h:182-196) as
//   pgp_super4pcs_hypotheses_gated: a model pair enters a base edge's list only when its normals stand to each other as the
//   edge's do.  It prints the quads the join makes with and without the gate.
// Usage:  match_oriented [seed]                     a synthetic object, checked against its known pose, ends "OK"
//         match_oriented segment.txt model.txt      "x y z nx ny nz" per line; the model is searched and scored
// The synthetic object is match_classic's box with a cylinder on top.  Its 300-point model is the search model and the
// validation model; the segment is the camera-facing part of those points under a seeded pose with 0.3 mm of noise, its
// normals the rotated model normals with N(0, 0.05) added to every component.
#include <pgp.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
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

bool read_cloud(const char* path, std::vector<float>* xyz, std::vector<float>* nrm) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  float p[6];
  while (std::fscanf(f, "%f %f %f %f %f %f%*[^\n]", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5]) == 6) {
    xyz->insert(xyz->end(), p, p + 3);
    nrm->insert(nrm->end(), p + 3, p + 6);
  }
  std::fclose(f);
  return !xyz->empty();
}

// the quads of the join over the pair lists the last chain call left resident: base b has lists 2 b and 2 b + 1
int resident_quads(pgp_ctx* ctx, const std::vector<float>& P, const std::vector<int>& base_ids, const std::vector<float>& inv,
                   int n_bases, float eps, long long* total) {
  std::vector<float> xyz(12 * (size_t)n_bases);
  std::vector<int> lists(2 * (size_t)n_bases), n_quads((size_t)n_bases);
  for (int b = 0; b < n_bases; ++b) {
    for (int k = 0; k < 4; ++k)
      for (int c = 0; c < 3; ++c) xyz[12 * (size_t)b + 3 * k + c] = P[3 * (size_t)base_ids[4 * (size_t)b + k] + c];
    lists[2 * (size_t)b] = 2 * b;
    lists[2 * (size_t)b + 1] = 2 * b + 1;
  }
  const int rc = pgp_find_congruent_batch_lists(ctx, xyz.data(), inv.data(), lists.data(), n_bases, eps, n_quads.data());
  *total = 0;
  for (int q : n_quads) *total += q;
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<float> P, Pn, M, Mn;   // segment, model, and their normals
  bool synthetic = argc < 3;
  float gt[16] = {0};
  if (synthetic) {
    std::mt19937 g(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    sample_surface(g, 300, &M, &Mn);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::normal_distribution<float> noise(0.f, 0.0003f), tilt(0.f, 0.05f);
    float ax[3] = {u(g), u(g), u(g)};
    const float al = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    for (float& a : ax) a /= al;
    const float ang = 0.35f + 2.4f * (0.5f + 0.5f * u(g)), c = std::cos(ang), s = std::sin(ang), C = 1.f - c;
    const float Rt[9] = {c + ax[0] * ax[0] * C,         ax[0] * ax[1] * C - ax[2] * s, ax[0] * ax[2] * C + ax[1] * s,
                         ax[1] * ax[0] * C + ax[2] * s, c + ax[1] * ax[1] * C,         ax[1] * ax[2] * C - ax[0] * s,
                         ax[2] * ax[0] * C - ax[1] * s, ax[2] * ax[1] * C + ax[0] * s, c + ax[2] * ax[2] * C};
    const float tt[3] = {0.02f * u(g), 0.02f * u(g), 0.6f};
    for (size_t i = 0; i < M.size() / 3; ++i) {
      float p[3], q[3];
      for (int r = 0; r < 3; ++r) {
        p[r] = Rt[3 * r] * M[3 * i] + Rt[3 * r + 1] * M[3 * i + 1] + Rt[3 * r + 2] * M[3 * i + 2] + tt[r];
        q[r] = Rt[3 * r] * Mn[3 * i] + Rt[3 * r + 1] * Mn[3 * i + 1] + Rt[3 * r + 2] * Mn[3 * i + 2];
      }
      if (q[0] * p[0] + q[1] * p[1] + q[2] * p[2] >= 0.f) continue;   // faces away from the camera at the origin
      for (int r = 0; r < 3; ++r) P.push_back(p[r] + noise(g));
      for (int r = 0; r < 3; ++r) Pn.push_back(q[r] + tilt(g));
    }
    for (int r = 0; r < 3; ++r) {   // the true pose, column-major
      for (int k = 0; k < 3; ++k) gt[4 * k + r] = Rt[3 * r + k];
      gt[12 + r] = tt[r];
    }
    gt[15] = 1.f;
  } else if (!read_cloud(argv[1], &P, &Pn) || !read_cloud(argv[2], &M, &Mn)) {
    std::printf("cannot read %s / %s (x y z nx ny nz per line)\n", argv[1], argv[2]);
    return 1;
  }
  const int nP = (int)P.size() / 3, nM = (int)M.size() / 3;
  // the model's diameter: the bound on a base's edges (the reference estimates it from 1000 random pairs, base.cc:274-287)
  float diameter = 0.f;
  for (int i = 0; i < nM; ++i)
    for (int j = 0; j < i; ++j) {
      const float d[3] = {M[3 * i] - M[3 * j], M[3 * i + 1] - M[3 * j + 1], M[3 * i + 2] - M[3 * j + 2]};
      diameter = std::max(diameter, std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
    }
  // the frames of Match4PCSBase::init: the segment minus its centroid, the model minus its own
  std::vector<float> V(M);   // the validation model: the same points
  float cP[3], cQ[3];
  CHECK(pgp_center(P.data(), nP, M.data(), nM, V.data(), nM, cP, cQ));
  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  CHECK(pgp_set_scene(ctx, P.data(), Pn.data(), nullptr, nP, 0.005f));
  CHECK(pgp_set_model(ctx, V.data(), nullptr, nM));
  CHECK(pgp_set_search_model(ctx, M.data(), nM));
  CHECK(pgp_set_search_model_attributes(ctx, Mn.data(), nullptr, nM));
  pgp_super4pcs_options opt;
  CHECK(pgp_super4pcs_default_options(&opt));
  opt.seed = 1;
  opt.max_base_diameter = diameter;
  const size_t cap = (size_t)opt.n_bases * (size_t)opt.max_per_base;
  std::vector<float> T(cap * 16), scores(cap), best_T(16);
  std::vector<int> status(cap), base_ids(4 * (size_t)opt.n_bases);
  std::vector<float> inv(2 * (size_t)opt.n_bases);
  std::vector<double> best_pose(16);
  int n_bases = 0, n_hyp = 0, best = -1;
  float best_score = 0.f;
  long long quads_plain = 0, quads_gated = 0;
  // without the gate, for the count alone: the same bases (the gates do not touch their selection)
  CHECK(pgp_super4pcs_hypotheses(ctx, &opt, cP, cQ, &n_bases, base_ids.data(), inv.data(), &n_hyp, T.data(), nullptr, status.data(),
                                 scores.data(), nullptr, &best, &best_score, best_T.data(), best_pose.data()));
  CHECK(resident_quads(ctx, P, base_ids, inv, n_bases, opt.eps, &quads_plain));
  pgp_pair_gates gates;
  CHECK(pgp_pair_gates_default(&gates));
  gates.max_normal_difference = 20.f;
  CHECK(pgp_super4pcs_hypotheses_gated(ctx, &opt, &gates, cP, cQ, &n_bases, base_ids.data(), inv.data(), &n_hyp, T.data(), nullptr,
                                       status.data(), scores.data(), nullptr, &best, &best_score, best_T.data(), best_pose.data()));
  CHECK(resident_quads(ctx, P, base_ids, inv, n_bases, opt.eps, &quads_gated));
  std::printf("segment %d points, model %d, diameter %.4f: %d bases, %d hypotheses, best %d (score %.4f)\n", nP, nM, diameter,
              n_bases, n_hyp, best, best_score);
  std::printf("quads: %lld with the 20 degree normal gate, %lld without\n", quads_gated, quads_plain);
  if (best < 0) {
    std::printf("no hypothesis scored above 0\n");
    return 1;
  }
  std::printf("pose (model -> segment, row-major):\n");
  for (int r = 0; r < 4; ++r)
    std::printf("  % .6f % .6f % .6f % .6f\n", best_pose[r], best_pose[4 + r], best_pose[8 + r], best_pose[12 + r]);
  if (synthetic) {
    float pose_f[16], rot = 0.f, trans = 0.f;
    const float sym[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 16; ++k) pose_f[k] = (float)best_pose[k];
    CHECK(pgp_pose_error(ctx, pose_f, gt, 1, sym, &rot, &trans));
    std::printf("against the true pose: %.2f deg, %.2f mm\n", rot, 1000.f * trans);
    if (!(rot <= 5.f && trans <= 0.01f)) {
      std::printf("FAIL: the best pose is off\n");
      return 1;
    }
  }
  CHECK(pgp_destroy(ctx));
  std::printf("OK\n");
  return 0;
}
