// csrc/base_device.h -- device functions that more than one base-selection kernel uses, stated once:
//   ppfk::fit_plane / seg_seg / try_quadrilateral   the plane through three base points (base.cc:527-547, :731-745), distSegmentToSegment
//                                                   (:81-148) and TryQuadrilateral (:415-464): base_select.hip (StoCS, pgp_base_invariants)
//                                                   and super4pcs.hip (SelectQuadrilateral)
//   v4dev::widest_triangle                           SelectRandomTriangle (:377-410) with the counter-based draw: v4pcs.hip and super4pcs.hip
#pragma once

#include "pgp_internal.h"
#include "ppf_key.h"

namespace pgp {
namespace ppfk {

struct Plane {
  float denom, A, B, C;
};
__device__ __forceinline__ Plane fit_plane(V3 q1, V3 q2, V3 q3) {  // base.cc:731-745, double arithmetic
  const double x1 = q1.x, y1 = q1.y, z1 = q1.z, x2 = q2.x, y2 = q2.y, z2 = q2.z, x3 = q3.x, y3 = q3.y, z3 = q3.z;
  Plane p;
  p.denom = (float)(-x3 * y2 * z1 + x2 * y3 * z1 + x3 * y1 * z2 - x1 * y3 * z2 - x2 * y1 * z3 + x1 * y2 * z3);
  const double dd = (double)p.denom;
  p.A = (float)((-y2 * z1 + y3 * z1 + y1 * z2 - y3 * z2 - y1 * z3 + y2 * z3) / dd);
  p.B = (float)((x2 * z1 - x3 * z1 - x1 * z2 + x3 * z2 + x1 * z3 - x2 * z3) / dd);
  p.C = (float)((-x2 * y1 + x3 * y1 + x1 * y2 - x3 * y2 - x1 * y3 + x2 * y3) / dd);
  return p;
}

// Closest approach of the segments P(s) = p1 + s u and Q(t) = q1 + t v, s, t in [0, 1]: the parameters
// are kept as fractions sN / sD and tN / tD of the 2 x 2 system's determinant and clamped edge by edge
// (the classic closed form the reference's distSegmentToSegment follows, base.cc:81-148).  Arithmetic
// as TryQuadrilateral instantiates it: float dot products widened to double, double fractions, the
// invariants narrowed to float before the residual vector is formed.  Returns |w + s u - t v|.
__device__ inline float seg_seg(V3 p1, V3 p2, V3 q1, V3 q2, double* invariant1, double* invariant2) {
  const double tiny = 0.0001;
  const V3 u = vsub(p2, p1), v = vsub(q2, q1), w = vsub(p1, q1);
  const double uu = dot_eigen(u, u), uv = dot_eigen(u, v), vv = dot_eigen(v, v), uw = dot_eigen(u, w), vw = dot_eigen(v, w);
  const double det = uu * vv - uv * uv;
  double sN, sD = det, tN, tD = det;
  if (det < tiny) {            // (almost) parallel: pin s = 0 and project q-side only
    sN = 0.0;
    sD = 1.0;
    tN = vw;
    tD = vv;
  } else {                      // interior solution of the unconstrained problem, then the s-edges
    sN = uv * vw - vv * uw;
    tN = uu * vw - uv * uw;
    if (sN < 0.0) {
      sN = 0.0;
      tN = vw;
      tD = vv;
    } else if (sN > sD) {
      sN = sD;
      tN = vw + uv;
      tD = vv;
    }
  }
  if (tN < 0.0) {               // t-edges: re-solve s on the edge t = 0 or t = 1
    tN = 0.0;
    const double m = -uw;
    if (m < 0.0) sN = 0.0;
    else if (m > uu) sN = sD;
    else {
      sN = m;
      sD = uu;
    }
  } else if (tN > tD) {
    tN = tD;
    const double m = -uw + uv;
    if (m < 0.0) sN = 0;
    else if (m > uu) sN = sD;
    else {
      sN = m;
      sD = uu;
    }
  }
  *invariant1 = fabs(sN) < tiny ? 0.0 : sN / sD;
  *invariant2 = fabs(tN) < tiny ? 0.0 : tN / tD;
  const float fs = (float)*invariant1, ft = (float)*invariant2;   // Eigen narrows the double scalars
  const V3 r = {sub(add(w.x, mul(fs, u.x)), mul(ft, v.x)), sub(add(w.y, mul(fs, u.y)), mul(ft, v.y)),
                sub(add(w.z, mul(fs, u.z)), mul(ft, v.z))};
  return norm_eigen(r);
}

// TryQuadrilateral on lanes 0..11 of the calling wave (all 64 lanes call): pairing p enumerates
// (i, j) in the reference's loop order; the first minimum wins (strict <).
__device__ inline bool try_quadrilateral(const float4* __restrict__ P, int ids[4], float* inv1, float* inv2) {
  const int lane = threadIdx.x & 63;
  const int p = lane < 12 ? lane : 0;
  const int i = p / 3;
  int j = p % 3;
  j += j >= i ? 1 : 0;
  int k = 0;
  while (k == i || k == j) k++;
  int l = 0;
  while (l == i || l == j || l == k) l++;
  V3 q[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) q[t] = ld3(P, ids[t]);
  auto pick = [&](int t) { return t == 0 ? q[0] : (t == 1 ? q[1] : (t == 2 ? q[2] : q[3])); };
  double li1, li2;
  float sd = seg_seg(pick(i), pick(j), pick(k), pick(l), &li1, &li2);
  if (lane >= 12 || !(sd == sd)) sd = __int_as_float(0x7F800000);   // NaN never passes `<`
  // arg-min with the lowest pairing index on ties: key = (distance bits, pairing)
  unsigned long long key = ((unsigned long long)__float_as_uint(sd) << 8) | (unsigned)p;   // sd >= 0
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o < key ? o : key;
  }
  key = __shfl(key, 0, 64);   // lanes 0..15 hold the minimum of lanes 0..15
  const int bp = (int)(key & 0xFFu);
  const bool valid = (key >> 8) < 0x7F800000ull && (key >> 8) < (unsigned long long)__float_as_uint(3.4028234663852886e38f);
  const float f1 = __shfl((float)li1, bp, 64), f2 = __shfl((float)li2, bp, 64);
  if (valid) {   // min_distance starts at FLT_MAX: a pairing at exactly FLT_MAX or beyond never wins
    const int bi = bp / 3;
    int bj = bp % 3;
    bj += bj >= bi ? 1 : 0;
    int bk = 0;
    while (bk == bi || bk == bj) bk++;
    int bl = 0;
    while (bl == bi || bl == bj || bl == bk) bl++;
    const int t0 = ids[0], t1 = ids[1], t2 = ids[2], t3 = ids[3];
    auto sel = [&](int t) { return t == 0 ? t0 : (t == 1 ? t1 : (t == 2 ? t2 : t3)); };
    ids[0] = sel(bi);
    ids[1] = sel(bj);
    ids[2] = sel(bk);
    ids[3] = sel(bl);
    *inv1 = f1;
    *inv2 = f2;
  }
  return valid;   // false: no pairing below FLT_MAX (the reference returns false); ids and invariants are left alone
}

}  // namespace ppfk

// The position-only modes (v4pcs.hip, super4pcs.hip SelectQuadrilateral): their dot products and squared norms are
// (x x + y y) + z z, exact_f32.h's _lr forms.
namespace v4dev {

using namespace exact;

// The widest triangle among trials first, first + stride, ... < T of the attempt whose stream is `st`, first point p0:
// key = how_wide bits << 32 | ~trial (how_wide > 0: its bits order as the floats do), 0 when no trial qualifies.  The greatest
// key over all the trials of an attempt is the reference's choice: the greatest width, then the first trial.
__device__ __forceinline__ unsigned long long widest_triangle(const float4* __restrict__ P, unsigned un, unsigned long long st, int T,
                                                              float DD, V3 p0, int first, int stride) {
  unsigned long long best = 0ull;
  for (int i = first; i < T; i += stride) {
    const int s = (int)(sample_variate(st, 1 + 2 * i) % un), t = (int)(sample_variate(st, 2 + 2 * i) % un);
    const V3 u = vsub(ld3(P, s), p0), w = vsub(ld3(P, t), p0);
    const V3 c = cross(u, w);
    const float how_wide = norm_lr(c);
    if (how_wide > 0.f && sqnorm_lr(u) < DD && sqnorm_lr(w) < DD) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(how_wide) << 32) | (0xFFFFFFFFu - (unsigned)i);
      best = key > best ? key : best;
    }
  }
  return best;
}
__device__ __forceinline__ int triangle_trial(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

}  // namespace v4dev
}  // namespace pgp
