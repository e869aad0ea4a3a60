// csrc/nn_prune.h -- which entries of a cell's candidate list can never be the NEAREST scene point of a query
// in that cell: pure arithmetic, host and device (grid_index.hip prunes with it; plain g++ compiles it,
// tools/nn_prune_check.cc and tests/test_nn_prune_cpu.py pin it).
//
// A cell's list (grid_index.hip) holds every scene point within `reach` of the cell's box B.  The scoring
// kernels ask a list for the nearest point within delta (weighted) or for any point within delta (plain).
// Candidate a is DOMINATED by candidate b of the same list when
//
//     min over x in B+ of ( |x - a|^2 - |x - b|^2 )  >  m                                              (*)
//
//   B+  B inflated per side by reach - delta, the slack choose_grid grants the float rounding of cell(x):
//       every position a kernel looks up in this cell lies in B+.  (Positions the kernels CLAMP or alias
//       into a cell from outside the grid are farther than delta from every scene point: no entry of the
//       full list passes their distance test, so no entry of a subset does.)
//   min |x - a|^2 - |x - b|^2 = 2 x . (b - a) + |a|^2 - |b|^2 is linear in x, so its minimum over the cube B+ of
//       centre c and edge e is the value at c minus e * sum_i |a_i - b_i|.
//   m   twice the float error of the kernels' sqdist (lcp_score.hip): d = fl(x - p) = (x - p)(1 + e1), its
//       square rounded once = (x - p)^2 (1 + e1)^2 (1 + e2), then fl(dy^2 + dz^2) and fl(dx^2 + ...) add one
//       rounding each: every term carries at most five factors (1 + e), |e| <= u = 2^-24, all terms are >= 0,
//       so |sqdist_float - sqdist_exact| <= ((1 + u)^5 - 1) d^2 < 5.000001 u d^2 -- beside a product that
//       falls below the normal range, whose error is at most 2^-150 each.  A candidate lies within reach of B
//       and a query inside B+, so d <= Dmax = reach + diagonal(B+), and twice the error is < 10.01 u Dmax^2.
//       m = 64 u Dmax^2: more than six times the bound (5.9e-10 m^2 at delta = 5 mm), and far above 2^-148.
//
// With (*), the kernels' float sqdist(x, b) < sqdist(x, a) STRICTLY for every query x of the cell, so
//   - a never holds the minimum key and never ties it (nearest, and the exact-ties flag);
//   - whenever a passes d2 <= delta^2, so does b (any);
//   - two candidates that tie at the minimum for some x do not dominate one another (the minimum in (*) is
//     then <= 0), duplicated points (same coordinates, two ids) neither: both stay.
// (*) with m > 0 is transitive and irreflexive: all dominated entries of a list go at once, and at least one
// entry of every list stays.  Evaluated in double: the candidates are floats, their differences are exact
// there and the rest rounds at 2^-53 of a coordinate times a list's extent -- 1e-16 m^2 in a scene 40 m from
// its origin, six orders of magnitude inside m.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define PGP_NNP_HD __host__ __device__
#else
#define PGP_NNP_HD
#endif

namespace pgp {
namespace nnp {

// B+ of one cell and the margin m of its lists
struct CellBox {
  double cx, cy, cz;   // centre of the cell's box
  double edge;         // edge of B+: h + 2 (reach - delta)
  double margin;       // m
};

// u = 2^-24, the unit round-off of float
constexpr double kUnitRoundoff = 1.0 / 16777216.0;
constexpr double kMarginFactor = 64.0;

// the box of cell (x, y, z) of a grid with origin (ox, oy, oz) and cell edge h, as the index build states it
// (grid_index.hip for_cells_in_reach: [o + k h, o + k h + h] per axis)
PGP_NNP_HD inline CellBox cell_box(float ox, float oy, float oz, float h, float reach, float delta, int x, int y, int z) {
  CellBox b;
  const double hd = (double)h, slack = (double)reach - (double)delta;
  b.cx = (double)ox + ((double)x + 0.5) * hd;
  b.cy = (double)oy + ((double)y + 0.5) * hd;
  b.cz = (double)oz + ((double)z + 0.5) * hd;
  b.edge = hd + 2.0 * slack;
  const double dmax = (double)reach + 1.7320508075688774 * b.edge;   // reach + diagonal of B+ (sqrt 3, rounded up)
  b.margin = kMarginFactor * kUnitRoundoff * dmax * dmax;
  return b;
}

// (*): candidate (ax, ay, az) is farther than candidate (bx, by, bz) from every position of B+, by more than m
PGP_NNP_HD inline bool dominated_by(const CellBox& c, double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = bx - ax, dy = by - ay, dz = bz - az;
  // |c - a|^2 - |c - b|^2 = sum_i (b_i - a_i)(2 c_i - a_i - b_i)
  const double at_centre = dx * (2.0 * c.cx - ax - bx) + dy * (2.0 * c.cy - ay - by) + dz * (2.0 * c.cz - az - bz);
  const double l1 = fabs(dx) + fabs(dy) + fabs(dz);
  return at_centre - c.edge * l1 > c.margin;
}

}  // namespace nnp
}  // namespace pgp
