// examples/settle_thin_plates.cc -- the three contact modes of the physics settling through the C ABI alone.
// Two scenes that the edge-edge rule's `reach` (1 cm) was not made for:
//   two 20 x 4 cm plates 2 mm thick (thinner than reach), crossed, the upper one dropped from 1 cm above the lower one;
//   two crossed 20 x 4 x 4 cm bars, the upper one started 3 cm inside the lower one (deeper than reach).
// The static body stands on the table.  Settled three times: with vertex-face contacts (the default), with
// pgp_physics_set_edge_contacts, and with pgp_physics_set_polyhedral_contacts (a separating-axis test with face
// clipping, no reach).  Prints the rest heights of all three and exits non-zero unless the polyhedral ones are the
// stacked half extents plus both margins, within one margin (1 mm).
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
  const float plate_h = 0.001f, bar_h = 0.02f;
  const int plate = add_box(ctx, 0.10f, 0.02f, plate_h), bar = add_box(ctx, 0.10f, 0.02f, bar_h);
  std::vector<int> offsets(2 * PGP_PHYSICS_MAX_VERTICES + 1), loops(2 * PGP_PHYSICS_MAX_EDGES);
  int n_faces = 0;
  CHECK(pgp_physics_shape_faces(ctx, plate, offsets.data(), loops.data(), &n_faces));
  std::printf("the plate's hull has %d faces; the first runs through vertices", n_faces);
  for (int k = offsets[0]; k < offsets[1]; ++k) std::printf(" %d", loops[k]);
  std::printf("\n");

  // state 0: the crossed plates, 1 cm apart; state 1: the crossed bars, 3 cm inside each other.  World-frame poses
  // (cam_pose NULL), the table top at z = 0.
  const float table[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.2f};
  const int dyn[2] = {plate, bar}, off[3] = {0, 1, 2}, ss[2] = {plate, bar};
  const float half[2] = {plate_h, bar_h}, start[2] = {3.f * plate_h + 0.01f, 3.f * bar_h - 0.03f};
  float T[32], sT[32], rest[2];
  for (int i = 0; i < 2; ++i) {
    pose(0.f, half[i], sT + 16 * i);
    pose(90.f, start[i], T + 16 * i);
    rest[i] = 3.f * half[i] + 2.f * MARGIN;
  }
  pgp_physics_options opt;
  CHECK(pgp_physics_default_options(&opt));
  float out[3][32];
  pgp_physics_info info[3][2];
  for (int mode = 0; mode < 3; ++mode) {
    CHECK(pgp_physics_set_edge_contacts(ctx, mode == 1, PGP_PHYSICS_EDGE_REACH_DEFAULT));
    CHECK(pgp_physics_set_polyhedral_contacts(ctx, mode == 2, PGP_PHYSICS_FACE_BIAS_DEFAULT));
    CHECK(pgp_physics_settle(ctx, &opt, 2, dyn, T, off, ss, sT, table, nullptr, out[mode], info[mode]));
  }
  CHECK(pgp_destroy(ctx));
  const char* what[2] = {"thin plates", "deep start"};
  int bad = 0;
  for (int i = 0; i < 2; ++i) {
    const float z = out[2][16 * i + 14];
    std::printf("%s: rests at %.4f vertex-face, %.4f edge-edge, %.4f polyhedral (constructed: %.4f; %d contacts, |v| %.1e)\n",
                what[i], out[0][16 * i + 14], out[1][16 * i + 14], z, rest[i], info[2][i].n_contacts, info[2][i].lin_speed);
    if (!(std::fabs(z - rest[i]) < MARGIN)) bad = 1, std::printf("  the polyhedral rest height is wrong\n");
  }
  if (bad) return 1;
  std::printf("OK\n");
  return 0;
}
