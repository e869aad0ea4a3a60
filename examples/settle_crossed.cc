// examples/settle_crossed.cc -- edge-edge contacts of the physics settling through the C ABI alone.
// Two scenes in which no vertex of either hull lies inside the other, so vertex-face contacts find nothing and the
// dropped body falls through to the table:
//   a 20 x 4 x 4 cm bar dropped across an identical bar, and a 10 cm cube dropped on an identical cube, yawed 45 deg.
// The static body stands on the table; the dynamic one starts with 1 cm between the hulls.  Settled twice, with
// pgp_physics_set_edge_contacts off (the default) and on; prints both rest heights and exits non-zero unless the
// switch-on ones are the stacked half extents plus both margins, within one margin (1 mm).
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

const float MARGIN = 0.001f;

int add_box(pgp_ctx* ctx, float hx, float hy, float hz) {
  std::vector<float> v;
  for (int i = 0; i < 8; ++i) {
    v.push_back(i & 1 ? hx : -hx);
    v.push_back(i & 2 ? hy : -hy);
    v.push_back(i & 4 ? hz : -hz);
  }
  int id = -1;
  CHECK(pgp_physics_add_shape(ctx, v.data(), 8, MARGIN, 256, &id));
  return id;
}

// world pose: yaw about +z, then the translation (column-major)
void pose(float yaw_deg, float z, float* T) {
  const float a = yaw_deg * 3.14159265f / 180.f, c = std::cos(a), s = std::sin(a);
  const float W[16] = {c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, 0, 0, z, 1};
  for (int k = 0; k < 16; ++k) T[k] = W[k];
}

}  // namespace

int main() {
  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  const float bar_h = 0.02f, cube_h = 0.05f;
  const int bar = add_box(ctx, 0.10f, 0.02f, bar_h), cube = add_box(ctx, cube_h, cube_h, cube_h);
  std::vector<int> rows(4 * PGP_PHYSICS_MAX_EDGES);
  int n_edges = 0;
  CHECK(pgp_physics_shape_edges(ctx, bar, rows.data(), &n_edges));
  std::printf("the bar's hull has %d edges; the first joins vertices %d and %d where planes %d and %d meet\n", n_edges,
              rows[0], rows[1], rows[2], rows[3]);

  // state 0: the crossed bars; state 1: the yawed cube.  World-frame poses (cam_pose NULL), the table top at z = 0.
  const float table[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.2f};
  const int dyn[2] = {bar, cube}, off[3] = {0, 1, 2}, ss[2] = {bar, cube};
  const float half[2] = {bar_h, cube_h}, yaw[2] = {90.f, 45.f};
  float T[32], sT[32], rest[2];
  for (int i = 0; i < 2; ++i) {
    pose(0.f, half[i], sT + 16 * i);
    pose(yaw[i], 3.f * half[i] + 0.01f, T + 16 * i);
    rest[i] = 3.f * half[i] + 2.f * MARGIN;
  }
  pgp_physics_options opt;
  CHECK(pgp_physics_default_options(&opt));
  float out[2][32];
  pgp_physics_info info[2][2];
  for (int on = 0; on < 2; ++on) {
    CHECK(pgp_physics_set_edge_contacts(ctx, on, PGP_PHYSICS_EDGE_REACH_DEFAULT));
    CHECK(pgp_physics_settle(ctx, &opt, 2, dyn, T, off, ss, sT, table, nullptr, out[on], info[on]));
  }
  CHECK(pgp_destroy(ctx));
  const char* what[2] = {"crossed bars", "yawed cube"};
  int bad = 0;
  for (int i = 0; i < 2; ++i) {
    const float z_off = out[0][16 * i + 14], z_on = out[1][16 * i + 14];
    std::printf("%s: rests at %.4f without edge contacts, %.4f with them (constructed: %.4f; %d contacts, |v| %.1e)\n",
                what[i], z_off, z_on, rest[i], info[1][i].n_contacts, info[1][i].lin_speed);
    if (!(std::fabs(z_on - rest[i]) < MARGIN)) bad = 1, std::printf("  the switch-on rest height is wrong\n");
  }
  if (bad) return 1;
  std::printf("OK\n");
  return 0;
}
