// examples/split_touching.cc -- two boxes pushed together on a table, told apart through the C ABI alone (include/pgp.h):
//   pgp_remove_table                  the table plane is fitted and its pixels zeroed
//   pgp_depth_components              what is left is ONE component: the boxes touch, no depth jump runs between them
//   pgp_depth_objects                 normals, the concave-crease cut, the cores' components and the growing: TWO
//   pgp_assign_masks_to_components    each object's 2-D mask falls into a component of its own, so each gets its own
//                                     search group
// The frame is synthetic: a camera 0.6 m above the table looking down at 45 degrees, a box 10 cm high and, pushed against
// its side, a box 5 cm high that stands 4 cm further back.  Where the low box's top and front meet the high box's side
// wall the surface has a concave crease; that is what the cut follows.  (Two boxes of equal height, flush side by side,
// would show no such crease: that contact is convex, and the method's limit.)  The program prints the group counts of
// both calls, checks one and two itself and ends with "OK".
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
struct Box {
  float lo[3], hi[3];   // world frame: the table is z = 0, the camera stands at (0, 0, 0.6)
  int cls;
};
// the boxes share the plane x = -0.18
const Box kBoxes[2] = {{{-0.30f, 0.52f, 0.f}, {-0.18f, 0.66f, 0.10f}, 1}, {{-0.18f, 0.56f, 0.f}, {-0.04f, 0.66f, 0.05f}, 2}};

// the ray origin + t dir against an axis-aligned box: the entry parameter, or a negative number
float hit_box(const float origin[3], const float dir[3], const Box& b) {
  float t_near = -1e30f, t_far = 1e30f;
  for (int k = 0; k < 3; ++k) {
    if (std::fabs(dir[k]) < 1e-9f) {
      if (origin[k] < b.lo[k] || origin[k] > b.hi[k]) return -1.f;
      continue;
    }
    const float t0 = (b.lo[k] - origin[k]) / dir[k], t1 = (b.hi[k] - origin[k]) / dir[k];
    t_near = std::max(t_near, std::min(t0, t1));
    t_far = std::min(t_far, std::max(t0, t1));
  }
  return t_near <= t_far && t_near > 0.f ? t_near : -1.f;
}

int groups_of(pgp_ctx* ctx, const std::vector<int>& ids, const std::vector<unsigned char>& classes, int rows, int cols,
              const char* name, int component[2], int pixels_in[2], int pixels_total[2]) {
  const int class_values[2] = {1, 2};
  int group[2];
  if (pgp_assign_masks_to_components(ctx, ids.data(), classes.data(), 1, rows, cols, class_values, 2, component, pixels_in,
                                     pixels_total, group) != PGP_OK) {
    std::printf("pgp_assign_masks_to_components failed (%s)\n", pgp_last_error());
    return -1;
  }
  const int n_groups = std::max(group[0], group[1]) + 1;
  std::printf("%s: %d group%s\n", name, n_groups, n_groups == 1 ? "" : "s");
  for (int o = 0; o < 2; ++o)
    std::printf("  object of class %d: component %d holds %d of its %d pixels, group %d\n", class_values[o], component[o],
                pixels_in[o], pixels_total[o], group[o]);
  return n_groups;
}
}  // namespace

int main(int argc, char** argv) {
  const int rows = 480, cols = 640;
  const float K[9] = {615.f, 0.f, 320.f, 0.f, 615.f, 240.f, 0.f, 0.f, 1.f};
  const float s = std::sqrt(0.5f);
  const float R[9] = {1.f, 0.f, 0.f, 0.f, -s, s, 0.f, -s, -s};   // camera -> world
  const float origin[3] = {0.f, 0.f, 0.6f};
  std::mt19937 gen(argc > 1 ? std::atoi(argv[1]) : 1);
  std::normal_distribution<float> noise(0.f, 0.0007f);
  const size_t n = (size_t)rows * cols;
  std::vector<float> depth(n);
  std::vector<unsigned char> classes(n, 0);
  for (int u = 0; u < rows; ++u)
    for (int v = 0; v < cols; ++v) {
      const float rc[3] = {(v - K[2]) / K[0], (u - K[5]) / K[4], 1.f};   // depth = the ray parameter
      float dir[3];
      for (int k = 0; k < 3; ++k) dir[k] = R[3 * k] * rc[0] + R[3 * k + 1] * rc[1] + R[3 * k + 2] * rc[2];
      float d = dir[2] < -1e-3f ? origin[2] / -dir[2] : 0.f;   // the table top
      for (const Box& b : kBoxes) {
        const float t = hit_box(origin, dir, b);
        if (t > 0.f && t < d) {
          d = t;
          classes[(size_t)u * cols + v] = (unsigned char)b.cls;
        }
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

  pgp_components_options copt;
  CHECK(pgp_components_default_options(&copt));
  pgp_crease_options crease;
  CHECK(pgp_crease_default_options(&crease));
  const int cap = 8;
  std::vector<int> ids(n);
  pgp_component_info info[cap];
  int component[2], pixels_in[2], pixels_total[2];

  // ---- touching objects are one component ----------------------------------------------------------------------------
  int plain[3] = {0, 0, 0};
  CHECK(pgp_depth_components(ctx, &copt, depth.data(), 0, nullptr, rows, cols, K, nullptr, ids.data(), info, cap, plain));
  std::printf("pgp_depth_components: %d kept of %d, %d valid pixels\n", plain[0], plain[1], plain[2]);
  const int plain_groups = groups_of(ctx, ids, classes, rows, cols, "pgp_depth_components", component, pixels_in, pixels_total);

  // ---- the concave crease between them cuts it -----------------------------------------------------------------------
  int counts[5] = {0, 0, 0, 0, 0};
  CHECK(pgp_depth_objects(ctx, &copt, &crease, depth.data(), 0, nullptr, rows, cols, K, nullptr, ids.data(), info, cap, counts));
  std::printf("pgp_depth_objects: %d kept of %d cores, %d valid pixels, %d crease pixels, %d labelled by growing\n", counts[0],
              counts[1], counts[2], counts[3], counts[4]);
  for (int k = 0; k < std::min(counts[0], cap); ++k)
    std::printf("  id %d: %d pixels, rows %d..%d, columns %d..%d, depth %.3f..%.3f\n", k + 1, info[k].pixels, info[k].u_min,
                info[k].u_max, info[k].v_min, info[k].v_max, info[k].z_min, info[k].z_max);
  const int cut_groups = groups_of(ctx, ids, classes, rows, cols, "pgp_depth_objects", component, pixels_in, pixels_total);
  CHECK(pgp_destroy(ctx));

  bool ok = plain[0] == 1 && plain_groups == 1 && counts[0] == 2 && cut_groups == 2 && counts[2] == plain[2] && counts[3] > 0;
  ok = ok && component[0] > 0 && component[1] > 0 && component[0] != component[1];
  for (int o = 0; o < 2; ++o) ok = ok && pixels_total[o] > 0 && pixels_in[o] >= 0.95 * pixels_total[o];
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
