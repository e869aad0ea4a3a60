// examples/remove_table.cc -- the node's table handling through the C ABI alone (include/pgp.h):
//   SceneCfg::removeTable    (PPE/data_layer/SceneCfg.cpp:38-82):  pgp_remove_table, one call
//   SceneCfg::getTableParams (SceneCfg.cpp:87-157):  the voxel cloud moved by camPose, pgp_fit_plane, the mean z of
//                            its inliers places the table model, pgp_icp_refine_ex (1 cm, 50 iterations) refines it.
// Usage:  remove_table [seed]                                   a synthetic 480 x 640 frame of a table and two boxes
//         remove_table depth.f32 rows cols fx fy cx cy          a float-metre depth image (raw row-major floats)
// The synthetic frame knows its table, so the program checks the results itself and ends with "OK".
#include <pgp.h>

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

int main(int argc, char** argv) {
  int rows = 480, cols = 640;
  float K[9] = {615.f, 0.f, 320.f, 0.f, 615.f, 240.f, 0.f, 0.f, 1.f};
  std::vector<float> depth;
  // camPose (world <- camera, row-major 3x3 + t): a camera 0.6 m above the table, looking down at 45 degrees
  const float s = std::sqrt(0.5f);
  const float R[9] = {1.f, 0.f, 0.f, 0.f, -s, s, 0.f, -s, -s};   // columns: camera x, y, z in the world
  const float C[3] = {0.7f, -0.6f, 0.6f};
  const bool synthetic = argc < 3;
  if (!synthetic) {
    if (argc < 8) {
      std::printf("usage: %s [seed] | depth.f32 rows cols fx fy cx cy\n", argv[0]);
      return 2;
    }
    rows = std::atoi(argv[2]);
    cols = std::atoi(argv[3]);
    K[0] = (float)std::atof(argv[4]);
    K[4] = (float)std::atof(argv[5]);
    K[2] = (float)std::atof(argv[6]);
    K[5] = (float)std::atof(argv[7]);
    depth.resize((size_t)rows * cols);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(depth.data(), 4, depth.size(), f) != depth.size()) {
      std::printf("cannot read %zu floats from %s\n", depth.size(), argv[1]);
      return 2;
    }
    std::fclose(f);
  } else {
    std::mt19937 gen(argc > 1 ? std::atoi(argv[1]) : 1);
    std::normal_distribution<float> noise(0.f, 0.0007f);
    depth.resize((size_t)rows * cols);
    for (int u = 0; u < rows; ++u)
      for (int v = 0; v < cols; ++v) {
        const float rc[3] = {(v - K[2]) / K[0], (u - K[5]) / K[4], 1.f};
        const float wz = R[6] * rc[0] + R[7] * rc[1] + R[8] * rc[2];   // world z of the ray
        float d = wz < -1e-3f ? -C[2] / wz : 0.f;                      // the table top is world z = 0
        if ((u > 120 && u < 200 && v > 180 && v < 300) || (u > 300 && u < 380 && v > 380 && v < 500)) d -= 0.06f;
        depth[(size_t)u * cols + v] = d > 0.f ? d + noise(gen) : 0.f;
      }
  }

  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  pgp_plane_options opt;
  CHECK(pgp_plane_default_options(&opt));

  // ---- removeTable: back-projection, 5 mm voxel grid, MSAC fit and the depth mask in one call ----------------------
  std::vector<float> masked = depth;
  float coeff[4];
  int n_masked = 0;
  CHECK(pgp_remove_table(ctx, masked.data(), 0, rows, cols, K, 0.005f, &opt, coeff, &n_masked));
  size_t n_valid = 0;
  for (float d : depth) n_valid += d > 0.1f && d < 2.0f;
  std::printf("removeTable: plane (%.5f %.5f %.5f %.5f), %d of %zu pixels zeroed\n", coeff[0], coeff[1], coeff[2], coeff[3],
              n_masked, n_valid);

  // ---- getTableParams: the voxel cloud (scene.ply) moved by camPose, the fit, the mean z of its inliers ----------
  std::vector<float> cloud((size_t)rows * cols * 3), vox((size_t)rows * cols * 3);
  int n_cloud = 0, n_vox = 0;
  CHECK(pgp_backproject_depth(ctx, depth.data(), 0, nullptr, rows, cols, K, 0.1, 2.0, cloud.data(), rows * cols, &n_cloud));
  CHECK(pgp_voxel_grid(ctx, cloud.data(), n_cloud, 0.005f, vox.data(), n_cloud, &n_vox));
  std::vector<float> scene((size_t)n_vox * 3);
  for (int i = 0; i < n_vox; ++i)
    for (int r = 0; r < 3; ++r)
      scene[3 * (size_t)i + r] = R[3 * r] * vox[3 * (size_t)i] + R[3 * r + 1] * vox[3 * (size_t)i + 1] +
                                 R[3 * r + 2] * vox[3 * (size_t)i + 2] + C[r];
  std::vector<unsigned char> inl(n_vox);
  int n_inl = 0;
  pgp_plane_info info;
  CHECK(pgp_fit_plane(ctx, scene.data(), n_vox, &opt, nullptr, 0, coeff, inl.data(), &n_inl, &info));
  double mean_z = 0.0;
  for (int i = 0; i < n_vox; ++i)
    if (inl[i]) mean_z += scene[3 * (size_t)i + 2];
  mean_z /= n_inl > 0 ? n_inl : 1;
  std::printf("getTableParams: %d voxels, %d inliers (candidate %d of %d evaluated), mean z %.5f\n", n_vox, n_inl,
              info.chosen, info.n_evaluated, mean_z);

  // the table model (a 1.4 m square top at model z = 0.2, 1 cm grid) placed at x = 0.7, z = mean_z - 0.2
  std::vector<float> table;
  for (int a = -70; a <= 70; ++a)
    for (int b = -70; b <= 70; ++b) {
      table.push_back(0.01f * a + 0.7f);
      table.push_back(0.01f * b);
      table.push_back(0.2f + (float)mean_z - 0.2f);
    }
  pgp_icp_options io;
  CHECK(pgp_icp_default_options(&io));
  io.max_iterations = 50;
  io.max_corr_dist = 0.01f;
  io.transformation_epsilon = 1e-9f;
  float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float energy = 0.f;
  int iters = 0;
  CHECK(pgp_icp_refine_ex(ctx, scene.data(), n_vox, table.data(), nullptr, (int)table.size() / 3, T, 1, &io, &energy, &iters));
  // tablePose = inverse(icp) * tablePose: the table top's height after the refinement
  const double top = mean_z - T[14];
  std::printf("table ICP: %d iterations, energy %.3g, translation (%.5f %.5f %.5f), table top z %.5f\n", iters, energy, T[12],
              T[13], T[14], top);
  CHECK(pgp_destroy(ctx));

  if (synthetic) {
    const double ang = std::acos(std::fmin(1.0, std::fabs((double)coeff[2]))) * 180.0 / M_PI;
    const bool ok = n_masked > 0.5 * n_valid && info.status == PGP_OK && ang < 1.0 && std::fabs(mean_z) < 0.002 &&
                    std::fabs(top) < 0.002 && n_inl > 0.5 * n_vox;
    std::printf("table normal %.3f deg from vertical, top at %.4f m (truth 0)\n", ang, top);
    if (!ok) {
      std::printf("FAILED\n");
      return 1;
    }
  }
  std::printf("OK\n");
  return 0;
}
