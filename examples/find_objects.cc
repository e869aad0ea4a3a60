// examples/find_objects.cc -- from a depth image to object proposals through the C ABI alone (include/pgp.h):
//   pgp_remove_table                  the table plane is fitted and its pixels zeroed (SceneCfg::removeTable)
//   pgp_depth_components              what is left falls into connected components (Euclidean clustering on the image)
//   pgp_component_mask_device + pgp_segment_from_depth_device   one segment cloud per component, made on the device
//   pgp_assign_masks_to_components    which component each object's 2-D mask falls into, and which objects could share
//                                     a search tree (HypothesisSelection.cpp:242-247 puts all of them into one)
// The frame is synthetic: a table seen at 45 degrees with four boxes on it, two apart and two touching.  Touching
// objects are ONE component -- the method's limit --, so the program expects three components and three groups, checks
// them itself and ends with "OK".
#include <pgp.h>
#include <hip/hip_runtime_api.h>

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
#define HCHECK(x)                                                                \
  do {                                                                           \
    if ((x) != hipSuccess) {                                                     \
      std::printf("%s failed\n", #x);                                            \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

namespace {
struct Box {
  int u0, u1, v0, v1, cls;
};
// rows [u0, u1), columns [v0, v1); boxes 3 and 4 share the edge v = 320
const Box kBoxes[4] = {{100, 170, 100, 200, 1}, {100, 170, 420, 520, 2}, {300, 380, 250, 320, 3}, {300, 380, 320, 400, 4}};
}  // namespace

int main(int argc, char** argv) {
  const int rows = 480, cols = 640;
  const float K[9] = {615.f, 0.f, 320.f, 0.f, 615.f, 240.f, 0.f, 0.f, 1.f};
  const float s = std::sqrt(0.5f);
  const float R[9] = {1.f, 0.f, 0.f, 0.f, -s, s, 0.f, -s, -s};   // a camera 0.6 m above the table, looking down at 45 degrees
  const float height = 0.6f;
  std::mt19937 gen(argc > 1 ? std::atoi(argv[1]) : 1);
  std::normal_distribution<float> noise(0.f, 0.0007f);
  const size_t n = (size_t)rows * cols;
  std::vector<float> depth(n);
  std::vector<unsigned char> classes(n, 0);
  for (int u = 0; u < rows; ++u)
    for (int v = 0; v < cols; ++v) {
      const float rc[3] = {(v - K[2]) / K[0], (u - K[5]) / K[4], 1.f};
      const float wz = R[6] * rc[0] + R[7] * rc[1] + R[8] * rc[2];
      float d = wz < -1e-3f ? height / -wz : 0.f;   // the table top
      for (const Box& b : kBoxes)
        if (u >= b.u0 && u < b.u1 && v >= b.v0 && v < b.v1) {
          d -= 0.06f;                                // a box top, 6 cm nearer along the ray
          classes[(size_t)u * cols + v] = (unsigned char)b.cls;
        }
      depth[(size_t)u * cols + v] = d > 0.f ? d + noise(gen) : 0.f;
    }

  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  pgp_plane_options popt;
  CHECK(pgp_plane_default_options(&popt));
  float coeff[4];
  int n_masked = 0;
  CHECK(pgp_remove_table(ctx, depth.data(), 0, rows, cols, K, 0.005f, &popt, coeff, &n_masked));
  std::printf("removeTable: plane (%.5f %.5f %.5f %.5f), %d pixels zeroed\n", coeff[0], coeff[1], coeff[2], coeff[3], n_masked);

  // ---- the components of what is left ------------------------------------------------------------------------------
  pgp_components_options copt;
  CHECK(pgp_components_default_options(&copt));
  const int cap = 8;
  std::vector<int> ids(n);
  pgp_component_info info[cap];
  int counts[3] = {0, 0, 0};
  CHECK(pgp_depth_components(ctx, &copt, depth.data(), 0, nullptr, rows, cols, K, nullptr, ids.data(), info, cap, counts));
  std::printf("components: %d kept of %d, %d valid pixels\n", counts[0], counts[1], counts[2]);
  const int n_comp = counts[0] < cap ? counts[0] : cap;
  for (int k = 0; k < n_comp; ++k)
    std::printf("  id %d: %d pixels, rows %d..%d, columns %d..%d, depth %.3f..%.3f, centroid (%.4f %.4f %.4f)\n", k + 1,
                info[k].pixels, info[k].u_min, info[k].u_max, info[k].v_min, info[k].v_max, info[k].z_min, info[k].z_max,
                info[k].sum_um[0] / 1e6 / info[k].pixels, info[k].sum_um[1] / 1e6 / info[k].pixels,
                info[k].sum_um[2] / 1e6 / info[k].pixels);

  // ---- one segment cloud per component, on the device --------------------------------------------------------------
  float* d_depth = nullptr;
  int* d_ids = nullptr;
  unsigned char* d_mask = nullptr;
  hipStream_t st = nullptr;
  HCHECK(hipStreamCreate(&st));
  HCHECK(hipMalloc((void**)&d_depth, n * 4));
  HCHECK(hipMalloc((void**)&d_ids, n * 4));
  HCHECK(hipMalloc((void**)&d_mask, n));
  HCHECK(hipMemcpy(d_depth, depth.data(), n * 4, hipMemcpyHostToDevice));
  HCHECK(hipMemcpy(d_ids, ids.data(), n * 4, hipMemcpyHostToDevice));
  pgp_segment_options sopt;
  CHECK(pgp_segment_default_options(&sopt));
  bool clouds_ok = true;
  for (int k = 0; k < n_comp; ++k) {
    int seg[4] = {0, 0, 0, 0}, installed = 0;
    float cP[3] = {0.f, 0.f, 0.f};
    CHECK(pgp_component_mask_device(ctx, d_ids, rows, cols, k + 1, d_mask, st));
    CHECK(pgp_segment_from_depth_device(ctx, &sopt, d_depth, 0, d_mask, rows, cols, K, nullptr, seg, &installed, cP, st));
    std::printf("  id %d: %d points back-projected, %d voxels, %d kept, scene %s\n", k + 1, seg[0], seg[1], seg[3],
                installed ? "installed" : "not installed");
    clouds_ok = clouds_ok && seg[0] == info[k].pixels && installed;
  }

  // ---- which component each object's mask falls into, and the search groups -----------------------------------------
  const int class_values[4] = {1, 2, 3, 4};
  int component[4], pixels_in[4], pixels_total[4], group[4];
  CHECK(pgp_assign_masks_to_components(ctx, ids.data(), classes.data(), 1, rows, cols, class_values, 4, component, pixels_in,
                                       pixels_total, group));
  int n_groups = 0;
  for (int o = 0; o < 4; ++o) {
    std::printf("  object of class %d: component %d holds %d of its %d pixels, group %d\n", class_values[o], component[o],
                pixels_in[o], pixels_total[o], group[o]);
    if (group[o] + 1 > n_groups) n_groups = group[o] + 1;
  }

  CHECK(pgp_destroy(ctx));
  HCHECK(hipFree(d_depth));
  HCHECK(hipFree(d_ids));
  HCHECK(hipFree(d_mask));
  HCHECK(hipStreamDestroy(st));

  bool ok = counts[0] == 3 && n_groups == 3 && clouds_ok;
  ok = ok && component[2] == component[3] && component[0] != component[1] && component[0] != component[2] &&
       component[1] != component[2] && component[0] > 0 && component[1] > 0 && component[2] > 0;
  for (int o = 0; o < 4; ++o) ok = ok && pixels_total[o] > 0 && pixels_in[o] >= 0.95 * pixels_total[o];
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
