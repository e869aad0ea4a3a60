// examples/match_classic.cc -- two position-only clouds in, a pose out, through the C ABI alone (include/pgp.h):
//   the matcher's classic mode (operMode 0, "Super4PCS": SelectQuadrilateral base.cc:505-580, two ExtractPairs per base
//   :1963-1969, FindCongruentQuadrilaterals, the fits and plain Verify of Perform_N_steps) as pgp_super4pcs_hypotheses.
//   No normals, no pair-feature table, no probability image.
// Usage:  match_classic [seed]                      a synthetic object, checked against its known pose, ends "OK"
//         match_classic segment.txt model.txt       "x y z" per line; the model is searched and scored
// The synthetic object is a box with a cylinder on top, off centre (no symmetry).  Its 300-point model is the search model
// and the validation model; the segment is the camera-facing part of those points under a seeded pose with 0.3 mm of
// noise and no clutter: wide bases reach for the extreme points of the segment, so the mode wants a clean one.
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

bool read_cloud(const char* path, std::vector<float>* xyz) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  float p[3];
  while (std::fscanf(f, "%f %f %f%*[^\n]", &p[0], &p[1], &p[2]) == 3) xyz->insert(xyz->end(), p, p + 3);
  std::fclose(f);
  return !xyz->empty();
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<float> P, M;   // segment, model
  bool synthetic = argc < 3;
  float gt[16] = {0};
  if (synthetic) {
    std::mt19937 g(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    std::vector<float> Mn;
    sample_surface(g, 300, &M, &Mn);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::normal_distribution<float> noise(0.f, 0.0003f);
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
    }
    for (int r = 0; r < 3; ++r) {   // the true pose, column-major
      for (int k = 0; k < 3; ++k) gt[4 * k + r] = Rt[3 * r + k];
      gt[12 + r] = tt[r];
    }
    gt[15] = 1.f;
  } else if (!read_cloud(argv[1], &P) || !read_cloud(argv[2], &M)) {
    std::printf("cannot read %s / %s (x y z per line)\n", argv[1], argv[2]);
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
  CHECK(pgp_set_scene(ctx, P.data(), nullptr, nullptr, nP, 0.005f));
  CHECK(pgp_set_model(ctx, V.data(), nullptr, nM));
  CHECK(pgp_set_search_model(ctx, M.data(), nM));
  pgp_super4pcs_options opt;
  CHECK(pgp_super4pcs_default_options(&opt));
  opt.seed = 1;
  opt.max_base_diameter = diameter;
  const size_t cap = (size_t)opt.n_bases * (size_t)opt.max_per_base;
  std::vector<float> T(cap * 16), scores(cap), best_T(16);
  std::vector<int> status(cap);
  std::vector<double> best_pose(16);
  int n_bases = 0, n_hyp = 0, best = -1;
  float best_score = 0.f;
  CHECK(pgp_super4pcs_hypotheses(ctx, &opt, cP, cQ, &n_bases, nullptr, nullptr, &n_hyp, T.data(), nullptr, status.data(),
                                 scores.data(), nullptr, &best, &best_score, best_T.data(), best_pose.data()));
  std::printf("segment %d points, model %d, diameter %.4f: %d bases, %d hypotheses, best %d (score %.4f)\n", nP, nM, diameter,
              n_bases, n_hyp, best, best_score);
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
