// examples/segment_in_hbm.cc -- a depth image becomes the scored scene without leaving HBM, through the C ABI alone:
//   pgp_segment_from_depth_device = back-projection -> voxel grid -> MLS normals -> radius filter + normal flip ->
//   centring -> weights from the probability image -> scene index (Segmentation.cpp:211-252,
//   ObjectPoseCandidateSet.cpp:28-51, base.cc:242-268,317-340), then pgp_score_lcp in PGP_MODE_WEIGHTED at once.
// The frame is synthetic: a curved patch 0.8 m in front of the camera, an elliptic object mask and a probability image
// that is 1 on the object.  The model is the patch itself, sampled on the host and centred on the centroid the call
// returns; of a handful of poses the identity must win.  Prints OK or exits non-zero.
#include <pgp.h>
#include <hip/hip_runtime_api.h>

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
#define HCHECK(x)                                                                         \
  do {                                                                                    \
    if ((x) != hipSuccess) {                                                              \
      std::fprintf(stderr, "%s failed\n", #x);                                            \
      std::exit(1);                                                                       \
    }                                                                                     \
  } while (0)

namespace {

const int ROWS = 240, COLS = 320;
const float FX = 300.f, FY = 300.f, CX = 160.f, CY = 120.f;

// depth of the patch at pixel (row u, column v): a shallow quadric
float depth_at(float u, float v) {
  const float a = (v - CX) / 100.f, b = (u - CY) / 100.f;
  return 0.8f + 0.03f * a * a - 0.02f * a * b + 0.025f * b * b;
}

bool on_object(int u, int v) {
  const float a = (v - CX) / 70.f, b = (u - CY) / 50.f;
  return a * a + b * b < 1.f;
}

void point_at(float u, float v, float p[3]) {
  const float z = depth_at(u, v);
  p[0] = (v - CX) * z / FX;
  p[1] = (u - CY) * z / FY;
  p[2] = z;
}

template <class T> T* upload(const std::vector<T>& h) {
  void* d = nullptr;
  HCHECK(hipMalloc(&d, h.size() * sizeof(T)));
  HCHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<T*>(d);
}

// column-major pose: rotation by `deg` about the x axis, then a translation
void pose(float deg, float tx, float ty, float tz, float* T) {
  const float a = deg * 3.14159265f / 180.f, c = std::cos(a), s = std::sin(a);
  const float M[16] = {1, 0, 0, 0, 0, c, s, 0, 0, -s, c, 0, tx, ty, tz, 1};
  for (int k = 0; k < 16; ++k) T[k] = M[k];
}

}  // namespace

int main() {
  std::vector<float> depth((size_t)ROWS * COLS);
  std::vector<unsigned char> mask((size_t)ROWS * COLS);
  std::vector<unsigned short> prob((size_t)ROWS * COLS);
  int n_mask = 0;
  for (int u = 0; u < ROWS; ++u)
    for (int v = 0; v < COLS; ++v) {
      const size_t i = (size_t)u * COLS + v;
      depth[i] = depth_at((float)u, (float)v);
      mask[i] = on_object(u, v) ? 1 : 0;
      prob[i] = mask[i] ? 10000 : 2000;
      n_mask += mask[i];
    }
  const float K[9] = {FX, 0, CX, 0, FY, CY, 0, 0, 1};

  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  float* d_depth = upload(depth);
  unsigned char* d_mask = upload(mask);
  unsigned short* d_prob = upload(prob);
  hipStream_t st = nullptr;
  HCHECK(hipStreamCreate(&st));

  pgp_segment_options opt;
  CHECK(pgp_segment_default_options(&opt));
  int counts[4] = {0, 0, 0, 0}, installed = 0;
  float cP[3] = {0, 0, 0};
  CHECK(pgp_segment_from_depth_device(ctx, &opt, d_depth, 0, d_mask, ROWS, COLS, K, d_prob, counts, &installed, cP, st));
  std::printf("back-projected %d, voxels %d, MLS rows %d, kept %d; centroid (%.4f, %.4f, %.4f)\n", counts[0], counts[1],
              counts[2], counts[3], cP[0], cP[1], cP[2]);
  if (!installed || counts[0] != n_mask || counts[3] <= opt.min_points || counts[3] > counts[1]) {
    std::fprintf(stderr, "no scene installed, or counts out of order\n");
    return 1;
  }
  if (std::fabs(cP[0]) > 0.01f || std::fabs(cP[1]) > 0.01f || std::fabs(cP[2] - 0.81f) > 0.02f) {
    std::fprintf(stderr, "the centroid is not the patch's\n");
    return 1;
  }

  // the model: the patch on every third pixel of the object, in the scene's centred frame, normals towards the camera
  std::vector<float> Q, Qn;
  for (int u = 1; u < ROWS - 1; u += 3)
    for (int v = 1; v < COLS - 1; v += 3) {
      if (!on_object(u, v)) continue;
      float p[3], pu[3], pv[3];
      point_at((float)u, (float)v, p);
      point_at((float)u + 1.f, (float)v, pu);
      point_at((float)u, (float)v + 1.f, pv);
      const float a[3] = {pu[0] - p[0], pu[1] - p[1], pu[2] - p[2]}, b[3] = {pv[0] - p[0], pv[1] - p[1], pv[2] - p[2]};
      float n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
      const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      const float s = (n[0] * p[0] + n[1] * p[1] + n[2] * p[2] > 0.f ? -1.f : 1.f) / len;
      for (int k = 0; k < 3; ++k) {
        Q.push_back(p[k] - cP[k]);
        Qn.push_back(n[k] * s);
      }
    }
  const int nQ = (int)(Q.size() / 3);
  CHECK(pgp_set_model(ctx, Q.data(), Qn.data(), nQ));

  // the identity, the patch pushed off its surface, tilted, and slid half its width
  const int n_h = 7;
  float T[n_h * 16];
  pose(0.f, 0.f, 0.f, 0.f, T);
  pose(0.f, 0.f, 0.f, 0.012f, T + 16);
  pose(0.f, 0.f, 0.f, -0.02f, T + 32);
  pose(25.f, 0.f, 0.f, 0.f, T + 48);
  pose(-40.f, 0.f, 0.f, 0.f, T + 64);
  pose(0.f, 0.10f, 0.f, 0.f, T + 80);
  pose(0.f, 0.f, -0.08f, 0.f, T + 96);
  float scores[n_h], best_score = 0.f;
  int inliers[n_h], best = -1;
  CHECK(pgp_score_lcp(ctx, T, n_h, PGP_MODE_WEIGHTED, 30.f, scores, inliers, &best, &best_score));
  for (int k = 0; k < n_h; ++k) std::printf("pose %d: weighted score %.4f\n", k, scores[k]);
  bool ok = best == 0 && best_score == scores[0] && scores[0] > 0.4f;
  for (int k = 1; k < n_h; ++k) ok = ok && scores[k] < 0.75f * scores[0];
  if (!ok) {
    std::fprintf(stderr, "the identity does not win (best %d, %.4f)\n", best, best_score);
    return 1;
  }

  CHECK(pgp_destroy(ctx));
  HCHECK(hipStreamDestroy(st));
  HCHECK(hipFree(d_depth));
  HCHECK(hipFree(d_mask));
  HCHECK(hipFree(d_prob));
  std::printf("OK\n");
  return 0;
}
