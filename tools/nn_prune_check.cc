// tools/nn_prune_check.cc -- the pruning rule of the nearest-only candidate lists (csrc/nn_prune.h) against what it
// promises, on the CPU: over random cells and random candidate lists, every float position of the (inflated) cell gets
// the same nearest candidate within delta, the same "any within delta" and the same number of candidates at the minimal
// distance from the pruned list as from the full one -- with the scoring kernels' own float arithmetic (lcp_score.hip
// sqdist: every operation rounded once; build with -ffp-contract=off).  Plain host code:
//   g++ -O1 -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] tools/nn_prune_check.cc -o nn_prune_check
// tests/test_nn_prune_cpu.py builds and runs it.  Usage: nn_prune_check [cells per scene] [positions per cell]
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../physimglobalpose_amd/csrc/nn_prune.h"

using pgp::nnp::CellBox;

struct Cand {
  float x, y, z;
  int id;
};

// lcp_score.hip sqdist
static float sqdist(float x, float y, float z, const Cand& p) {
  const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
  const float yy = dy * dy, zz = dz * dz, xx = dx * dx;
  const float yz = yy + zz;
  return xx + yz;
}

// grid_index.hip box_dist2
static float box_dist2(float px, float lo, float h) {
  const float a = lo - px, b = px - (lo + h);
  const float d = fmaxf(fmaxf(a, b), 0.f);
  return d * d;
}

struct Answer {
  uint64_t key;   // (bits of the minimal d2) << 32 | lowest id at it; ~0: none within delta
  int at_min;     // candidates at the minimal distance (the exact-ties flag fires on >= 2)
  bool any;
};

static Answer ask(const std::vector<Cand>& list, float x, float y, float z, float sq_eps) {
  Answer r{~0ull, 0, false};
  for (const Cand& c : list) {
    const float d2 = sqdist(x, y, z, c);
    if (!(d2 <= sq_eps)) continue;
    r.any = true;
    uint32_t bits;
    std::memcpy(&bits, &d2, 4);
    const uint64_t key = ((uint64_t)bits << 32) | (uint32_t)c.id;
    if (r.key == ~0ull || (key >> 32) < (r.key >> 32)) r.at_min = 1;
    else if ((key >> 32) == (r.key >> 32)) ++r.at_min;
    if (key < r.key) r.key = key;
  }
  return r;
}

static std::vector<char> keep_flags(const CellBox& box, const std::vector<Cand>& list) {
  std::vector<char> keep(list.size(), 1);
  for (size_t a = 0; a < list.size(); ++a)
    for (size_t b = 0; b < list.size(); ++b)
      if (pgp::nnp::dominated_by(box, list[a].x, list[a].y, list[a].z, list[b].x, list[b].y, list[b].z)) keep[a] = 0;
  return keep;
}

static long long g_failures = 0;
static void fail(const char* what, double base, int cell, int pos) {
  if (++g_failures <= 20) std::printf("FAIL %s (scene at %g, cell %d, position %d)\n", what, base, cell, pos);
}

// a float inside [lo, hi] (doubles): the nearest float, moved inwards when the rounding left the interval
static float inside(double v, double lo, double hi) {
  float f = (float)v;
  if ((double)f < lo) f = nextafterf(f, FLT_MAX);
  if ((double)f > hi) f = nextafterf(f, -FLT_MAX);
  return f;
}

int main(int argc, char** argv) {
  const int n_cells = argc > 1 ? atoi(argv[1]) : 200;
  const int n_pos = argc > 2 ? atoi(argv[2]) : 10000;
  std::mt19937_64 rng(20240607);
  auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
  const float delta = 0.005f, sq_eps = delta * delta, h = delta * 0.85f;
  long long n_full = 0, n_kept = 0, n_queries = 0, n_hits = 0, n_ties = 0;
  const double bases[2] = {0.5, 40.0};   // a table-top scene near its origin; a room-sized scene far from it
  for (const double base : bases) {
    // grid_index.hip choose_grid: the margin, hence the slack of B+ and Dmax, grow with the scene's coordinates
    const float maxabs = (float)base + 0.3f, maxext = base > 1.0 ? 5.f : 0.3f;
    const float margin = 0.004f * h + 1e-6f * 1024.f * h + 64.f * FLT_EPSILON * (maxabs + maxext);
    const float reach = delta * (1.f + 4.f * FLT_EPSILON) + margin;
    const int k0 = (int)std::floor((base - 0.2) / h);
    const float o = ((float)k0 - 0.5f) * h;   // origin on the lattice, the same on the three axes
    for (int cell = 0; cell < n_cells; ++cell) {
      const int cx = (int)uni(0, 90), cy = (int)uni(0, 90), cz = (int)uni(0, 90);
      const CellBox box = pgp::nnp::cell_box(o, o, o, h, reach, delta, cx, cy, cz);
      const float lo[3] = {o + (float)cx * h, o + (float)cy * h, o + (float)cz * h};
      // B+ stated here on its own (not read off the header's box): the cell inflated by reach - delta per side
      const double c[3] = {(double)o + (cx + 0.5) * (double)h, (double)o + (cy + 0.5) * (double)h, (double)o + (cz + 0.5) * (double)h};
      const double half = 0.5 * (double)h + ((double)reach - (double)delta);
      // 2 .. 40 candidates within reach of the box, as the build admits them; kinds of list: scattered in the whole
      // reach, on a noisy plane through the cell (a surface), with duplicates, with mirror pairs, with pairs at the
      // rule's threshold
      const int kind = cell % 5, n = 2 + (int)uni(0, 39);
      std::vector<Cand> list;
      double nrm[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
      const double nl = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]) + 1e-12;
      const double off = uni(-0.003, 0.003);
      while ((int)list.size() < n) {
        double p[3];
        for (int k = 0; k < 3; ++k) p[k] = c[k] + uni(-1, 1) * (0.5 * h + reach);
        if (kind == 1) {   // onto the plane n . (p - c) = off, 0.3 mm of noise
          double d = -off;
          for (int k = 0; k < 3; ++k) d += (p[k] - c[k]) * nrm[k] / nl;
          for (int k = 0; k < 3; ++k) p[k] -= (d + uni(-3e-4, 3e-4)) * nrm[k] / nl;
        }
        Cand q{(float)p[0], (float)p[1], (float)p[2], (int)(rng() % 1000000)};
        if (box_dist2(q.x, lo[0], h) + box_dist2(q.y, lo[1], h) + box_dist2(q.z, lo[2], h) > reach * reach) continue;
        list.push_back(q);
        if (kind == 2 && (int)list.size() < n && uni(0, 1) < 0.3) {   // the same coordinates under a second id
          q.id = (int)(rng() % 1000000);
          list.push_back(q);
        }
        if (kind == 4 && (int)list.size() < n && uni(0, 1) < 0.5) {
          // a partner at the rule's threshold: q mirrored in the plane that touches B+ at one corner only.  The corner is
          // then exactly as far from both (every other position is nearer the partner), up to the partner's rounding to
          // float -- the minimum of (*) lands within a few 1e-10 m^2 of zero, either side: where the margin decides
          double sg[3], s_n = 0.0;
          for (int k = 0; k < 3; ++k) sg[k] = uni(0, 1) < 0.5 ? -1.0 : 1.0;
          const double qq[3] = {q.x, q.y, q.z};
          for (int k = 0; k < 3; ++k) s_n += (qq[k] - (c[k] + half * sg[k])) * sg[k] / 1.7320508075688772;
          Cand m{(float)(qq[0] - 2.0 * s_n * sg[0] / 1.7320508075688772), (float)(qq[1] - 2.0 * s_n * sg[1] / 1.7320508075688772),
                 (float)(qq[2] - 2.0 * s_n * sg[2] / 1.7320508075688772), (int)(rng() % 1000000)};
          if (s_n > 1e-4 && box_dist2(m.x, lo[0], h) + box_dist2(m.y, lo[1], h) + box_dist2(m.z, lo[2], h) <= reach * reach) list.push_back(m);
        }
        if (kind == 3 && (int)list.size() < n && uni(0, 1) < 0.3) {   // its mirror image in the plane x = centre
          const float cxf = (float)c[0];
          Cand m = q;
          m.x = cxf + (cxf - q.x);
          m.id = (int)(rng() % 1000000);
          if (box_dist2(m.x, lo[0], h) + box_dist2(m.y, lo[1], h) + box_dist2(m.z, lo[2], h) <= reach * reach) list.push_back(m);
        }
      }
      const std::vector<char> keep = keep_flags(box, list);
      std::vector<Cand> pruned;
      for (size_t i = 0; i < list.size(); ++i)
        if (keep[i]) pruned.push_back(list[i]);
      n_full += (long long)list.size();
      n_kept += (long long)pruned.size();
      if (pruned.empty()) fail("a list lost every entry", base, cell, -1);
      for (size_t i = 0; i < list.size(); ++i)   // equal coordinates: kept together or dropped together
        for (size_t j = 0; j < i; ++j)
          if (list[i].x == list[j].x && list[i].y == list[j].y && list[i].z == list[j].z && keep[i] != keep[j])
            fail("one of two duplicated points was dropped", base, cell, -1);
      for (int p = 0; p < n_pos; ++p) {
        double t[3];
        for (int k = 0; k < 3; ++k) t[k] = uni(-1, 1);
        if (p < 8) {   // the corners of B+
          for (int k = 0; k < 3; ++k) t[k] = (p >> k) & 1 ? 1.0 : -1.0;
        } else if (p < 14) {   // the centres of its faces
          for (int k = 0; k < 3; ++k) t[k] = 0.0;
          t[(p - 8) >> 1] = (p & 1) ? 1.0 : -1.0;
        } else if (p % 4 == 0) {   // on a face
          t[p % 3] = (p & 4) ? 1.0 : -1.0;
        } else if (p % 4 == 1 && !list.empty()) {   // next to a candidate (the hits and the ties live there)
          const Cand& q = list[(size_t)p % list.size()];
          const double qq[3] = {q.x, q.y, q.z};
          for (int k = 0; k < 3; ++k) t[k] = std::fmin(1.0, std::fmax(-1.0, (qq[k] + uni(-0.004, 0.004) - c[k]) / half));
        }
        const float x = inside(c[0] + t[0] * half, c[0] - half, c[0] + half), y = inside(c[1] + t[1] * half, c[1] - half, c[1] + half),
                    z = inside(c[2] + t[2] * half, c[2] - half, c[2] + half);
        const Answer f = ask(list, x, y, z, sq_eps), g = ask(pruned, x, y, z, sq_eps);
        ++n_queries;
        n_hits += f.any;
        n_ties += f.at_min >= 2;
        if (f.key != g.key) fail("the nearest candidate differs", base, cell, p);
        if (f.any != g.any) fail("'any within delta' differs", base, cell, p);
        if (f.at_min != g.at_min) fail("the candidates at the minimal distance differ", base, cell, p);
      }
    }
  }
  // the two cases that must keep both entries, stated on their own
  {
    const float reach = delta * 1.01f, o = -0.5f * h;
    const CellBox box = pgp::nnp::cell_box(o, o, o, h, reach, delta, 3, 3, 3);
    const float cx = (float)box.cx;
    std::vector<Cand> dup = {{cx + 0.001f, (float)box.cy, (float)box.cz, 7}, {cx + 0.001f, (float)box.cy, (float)box.cz, 3}};
    std::vector<Cand> mir = {{cx + 0.001f, (float)box.cy, (float)box.cz, 7}, {cx - 0.001f, (float)box.cy, (float)box.cz, 3}};
    for (char k : keep_flags(box, dup))
      if (!k) fail("a duplicated pair lost an entry", 0.0, -1, -1);
    for (char k : keep_flags(box, mir))
      if (!k) fail("a mirror pair lost an entry", 0.0, -1, -1);
    // ... and one that must not: a point 1 mm from the cell against one 4 mm behind it
    std::vector<Cand> far = {{cx, (float)box.cy, (float)(box.cz + 0.5 * h + 0.001), 1}, {cx, (float)box.cy, (float)(box.cz + 0.5 * h + 0.005), 2}};
    const std::vector<char> k = keep_flags(box, far);
    if (!k[0] || k[1]) fail("the point behind a nearer one was kept", 0.0, -1, -1);
  }
  std::printf("lists: %lld entries, %lld kept (%.3f); %lld queries, %lld with a neighbour, %lld tied at the minimum\n", n_full, n_kept,
              n_full ? (double)n_kept / (double)n_full : 0.0, n_queries, n_hits, n_ties);
  if (n_kept >= n_full) fail("nothing was pruned", 0.0, -1, -1);
  if (n_hits == 0) fail("no query had a neighbour", 0.0, -1, -1);
  if (g_failures) {
    std::printf("%lld FAILURES\n", g_failures);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}
