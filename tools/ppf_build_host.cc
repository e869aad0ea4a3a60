// tools/ppf_build_host.cc -- the way to a pair-feature table without pgp_set_ppf_map_from_model, timed: the host
// double loop of examples/ppf_hypotheses.cc (computePPF of every ordered pair into a std::map, flattened to
// pgp_set_ppf_map's arrays) and the hand-over with pgp_set_ppf_map.  Driven by tools/ppf_build_time.py.
//   ppf_build_host cloud.f32 n loop_reps set_reps      (cloud.f32: n x 6 float32, x y z nx ny nz)
// prints "keys K pairs P", "loop_ms t ..." and "set_ms t ..." (the first pgp_set_ppf_map call is a warm-up, not listed).
#include <pgp.h>

#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

namespace {

int approximate_bin(int val, int disc) {   // base.cc:150-160
  const int lower = val - (val % disc), upper = lower + disc;
  return (val - lower < upper - val) ? lower : upper;
}

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

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: ppf_build_host cloud.f32 n loop_reps set_reps\n");
    return 2;
  }
  const int n = std::atoi(argv[2]), loop_reps = std::atoi(argv[3]), set_reps = std::atoi(argv[4]);
  std::vector<float> c((size_t)n * 6);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(c.data(), 4, c.size(), f) != c.size()) {
    std::fprintf(stderr, "cannot read %d points from %s\n", n, argv[1]);
    return 2;
  }
  std::fclose(f);
  std::vector<int> keys, counts, pairs;
  std::vector<double> loop_ms, set_ms;
  for (int rep = 0; rep < loop_reps; ++rep) {
    const double t0 = now_ms();
    std::map<std::array<int, 4>, std::vector<std::pair<int, int>>> table;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        if (i != j) table[ppf(&c[6 * (size_t)i], &c[6 * (size_t)i + 3], &c[6 * (size_t)j], &c[6 * (size_t)j + 3])].push_back(std::make_pair(i, j));
    keys.clear();
    counts.clear();
    pairs.clear();
    for (const auto& kv : table) {
      keys.insert(keys.end(), kv.first.begin(), kv.first.end());
      counts.push_back((int)kv.second.size());
      for (const auto& pr : kv.second) {
        pairs.push_back(pr.first);
        pairs.push_back(pr.second);
      }
    }
    loop_ms.push_back(now_ms() - t0);
  }
  pgp_ctx* ctx = nullptr;
  if (pgp_create(&ctx, -1) != PGP_OK) {
    std::fprintf(stderr, "pgp_create: %s\n", pgp_last_error());
    return 1;
  }
  for (int rep = 0; rep <= set_reps; ++rep) {
    const double t0 = now_ms();
    if (pgp_set_ppf_map(ctx, keys.data(), counts.data(), pairs.data(), (int)counts.size()) != PGP_OK) {
      std::fprintf(stderr, "pgp_set_ppf_map: %s\n", pgp_last_error());
      return 1;
    }
    if (rep) set_ms.push_back(now_ms() - t0);
  }
  pgp_destroy(ctx);
  std::printf("keys %zu pairs %zu\nloop_ms", counts.size(), pairs.size() / 2);
  for (double t : loop_ms) std::printf(" %.3f", t);
  std::printf("\nset_ms");
  for (double t : set_ms) std::printf(" %.3f", t);
  std::printf("\n");
  return 0;
}
