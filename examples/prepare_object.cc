// examples/prepare_object.cc -- a new object's PPFMap.txt through the C ABI alone (include/pgp.h): the step the node
// expects to have been done offline for every object (PPE/data_layer/Objects.cpp:31-49 reads the file; nothing in the
// node writes it).
//   pgp_set_ppf_map_from_model builds the pair-feature table of the search cloud on the device and installs it,
//   pgp_get_ppf_map reads it back, the program writes it in readPPFMap's format
//       f1 f2 f3 f4 count  i j  i j ...        (one key per line, keys in std::map order)
//   parses the file again the way readPPFMap does and checks it equals the device table, then runs pgp_select_bases
//   once on the installed table with the cloud itself as the segment.
// Usage:  prepare_object [cloud.txt | seed] [PPFMap.txt]
//   cloud.txt: one point per line, "x y z nx ny nz" in metres.  Without it a synthetic object (a box with a cylinder
//   on top, off centre) is sampled with 600 points.  Ends "OK".
#include <pgp.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <random>
#include <string>
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

// box 0.16 x 0.10 x 0.06 centred at the origin, cylinder of radius 0.025, height 0.06 on its top face at (0.04, 0.01)
void sample_surface(std::mt19937& g, int n, std::vector<float>* xyz, std::vector<float>* nrm) {
  std::uniform_real_distribution<float> u(0.f, 1.f);
  const float half[3] = {0.08f, 0.05f, 0.03f}, r = 0.025f, h = 0.06f, cx = 0.04f, cy = 0.01f;
  for (int i = 0; i < n; ++i) {
    float p[3], q[3] = {0.f, 0.f, 0.f};
    if (u(g) < 0.8f) {
      const int ax = (int)(3.f * u(g)) % 3;
      const float sgn = u(g) < 0.5f ? -1.f : 1.f;
      for (int k = 0; k < 3; ++k) p[k] = (2.f * u(g) - 1.f) * half[k];
      p[ax] = sgn * half[ax];
      q[ax] = sgn;
    } else {
      const float th = 6.2831853f * u(g);
      q[0] = std::cos(th);
      q[1] = std::sin(th);
      p[0] = cx + r * q[0];
      p[1] = cy + r * q[1];
      p[2] = half[2] + h * u(g);
    }
    for (int k = 0; k < 3; ++k) {
      xyz->push_back(p[k]);
      nrm->push_back(q[k]);
    }
  }
}

typedef std::map<std::vector<int>, std::vector<std::pair<int, int> > > PpfMap;

}  // namespace

int main(int argc, char** argv) {
  std::vector<float> M, Mn;
  std::ifstream cloud;
  if (argc > 1) cloud.open(argv[1]);
  if (cloud.is_open()) {
    float v[6];
    while (cloud >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5]) {
      M.insert(M.end(), v, v + 3);
      Mn.insert(Mn.end(), v + 3, v + 6);
    }
  } else {
    std::mt19937 g(argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u);
    sample_surface(g, 600, &M, &Mn);
  }
  const std::string out_path = argc > 2 ? argv[2] : "PPFMap.txt";
  const int n = (int)M.size() / 3;

  pgp_ctx* ctx = nullptr;
  CHECK(pgp_create(&ctx, -1));
  int n_keys = 0;
  long long n_pairs = 0;
  CHECK(pgp_set_ppf_map_from_model(ctx, M.data(), Mn.data(), n, &n_keys, &n_pairs));
  std::vector<int> keys((size_t)n_keys * 4 + 4), counts((size_t)n_keys + 1), pairs((size_t)n_pairs * 2 + 2);
  CHECK(pgp_get_ppf_map(ctx, keys.data(), counts.data(), pairs.data(), n_keys, n_pairs, &n_keys, &n_pairs));

  {   // PPFMap.txt
    std::ofstream f(out_path.c_str());
    size_t at = 0;
    for (int k = 0; k < n_keys; ++k) {
      f << keys[4 * k] << ' ' << keys[4 * k + 1] << ' ' << keys[4 * k + 2] << ' ' << keys[4 * k + 3] << ' ' << counts[k];
      for (int c = 0; c < counts[k]; ++c, ++at) f << ' ' << pairs[2 * at] << ' ' << pairs[2 * at + 1];
      f << '\n';
    }
    if (!f) {
      std::printf("cannot write %s\n", out_path.c_str());
      return 1;
    }
  }

  // the file as Objects::readPPFMap reads it
  PpfMap map;
  {
    std::ifstream f(out_path.c_str());
    std::vector<int> feature(4);
    int count = 0, a = 0, b = 0;
    while (f >> feature[0] >> feature[1] >> feature[2] >> feature[3] >> count) {
      std::vector<std::pair<int, int> > list;
      for (int c = 0; c < count; ++c) {
        f >> a >> b;
        list.push_back(std::make_pair(a, b));
      }
      map.insert(std::make_pair(feature, list));
    }
  }
  // ... equals the device table: same keys in the same (std::map) order, same pair lists
  bool same = (int)map.size() == n_keys;
  size_t at = 0;
  long long total = 0;
  int k = 0;
  for (PpfMap::const_iterator it = map.begin(); same && it != map.end(); ++it, ++k) {
    for (int c = 0; c < 4; ++c) same = same && it->first[c] == keys[4 * k + c];
    same = same && (int)it->second.size() == counts[k];
    for (size_t c = 0; same && c < it->second.size(); ++c, ++at)
      same = it->second[c].first == pairs[2 * at] && it->second[c].second == pairs[2 * at + 1];
    total += (long long)it->second.size();
  }
  if (!same || total != n_pairs) {
    std::printf("FAIL: %s does not read back as the device table (%zu keys, %lld pairs)\n", out_path.c_str(), map.size(), total);
    return 1;
  }

  // the installed table at work: one base selection with the cloud itself as the segment
  std::vector<float> w(n, 1.f);
  CHECK(pgp_set_scene(ctx, M.data(), Mn.data(), w.data(), n, 0.005f));
  const int attempts = 64;
  std::mt19937_64 eng(7);
  std::vector<double> u((size_t)attempts * 4);
  for (size_t i = 0; i < u.size(); ++i) u[i] = std::generate_canonical<double, 53>(eng);
  std::vector<int> ids((size_t)attempts * 4), status(attempts);
  std::vector<float> inv((size_t)attempts * 2);
  CHECK(pgp_select_bases(ctx, u.data(), attempts, ids.data(), inv.data(), status.data()));
  int found = 0;
  for (int i = 0; i < attempts; ++i) found += status[i] == 1;
  CHECK(pgp_destroy(ctx));
  std::printf("%d points -> %d keys, %lld pairs (of %lld ordered pairs) written to %s; %d of %d base selections found a base\n",
              n, n_keys, n_pairs, (long long)n * (n - 1), out_path.c_str(), found, attempts);
  if (found == 0) {
    std::printf("FAIL: no base on the object's own cloud\n");
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
