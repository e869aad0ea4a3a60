// csrc/eigen33.h -- pcl::eigen33 for a symmetric 3 x 3 matrix in double (smallest eigenvalue and its
// eigenvector), shared by the MLS normals (mls.hip) and the plane refit (plane.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace pgp {

// pcl::computeRoots2 / computeRoots (pcl/common/impl/eigen.hpp), double
__device__ __forceinline__ void roots2(double b, double c, double r[3]) {
  r[0] = 0.0;
  double d = b * b - 4.0 * c;
  if (d < 0.0) d = 0.0;   // no real roots: set to zero (numerical noise)
  const double sd = sqrt(d);
  r[2] = 0.5 * (b + sd);
  r[1] = 0.5 * (b - sd);
}

__device__ inline void roots3(const double m[6], double r[3]) {   // m = {xx, xy, xz, yy, yz, zz}
  const double c0 = m[0] * m[3] * m[5] + 2.0 * m[1] * m[2] * m[4] - m[0] * m[4] * m[4] - m[3] * m[2] * m[2] -
                    m[5] * m[1] * m[1];
  const double c1 = m[0] * m[3] - m[1] * m[1] + m[0] * m[5] - m[2] * m[2] + m[3] * m[5] - m[4] * m[4];
  const double c2 = m[0] + m[3] + m[5];
  if (fabs(c0) < DBL_EPSILON) {   // one root is 0 -> quadratic equation
    roots2(c2, c1, r);
    return;
  }
  const double s_inv3 = 1.0 / 3.0, s_sqrt3 = sqrt(3.0);
  const double c2_over_3 = c2 * s_inv3;
  double a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0) a_over_3 = 0.0;
  const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
  double q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0) q = 0.0;
  const double rho = sqrt(-a_over_3);
  const double theta = atan2(sqrt(-q), half_b) * s_inv3;
  const double cos_theta = cos(theta), sin_theta = sin(theta);
  r[0] = c2_over_3 + 2.0 * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  // sort in increasing order (PCL's three conditional swaps)
  if (r[0] >= r[1]) { const double t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] >= r[2]) {
    const double t = r[1]; r[1] = r[2]; r[2] = t;
    if (r[0] >= r[1]) { const double u = r[0]; r[0] = r[1]; r[1] = u; }
  }
  if (r[0] <= 0.0) roots2(c2, c1, r);   // a symmetric positive semi-definite matrix has no negative eigenvalue
}

// pcl::eigen33 (smallest eigenvalue + its eigenvector), double
__device__ inline void eigen33_smallest(const double cov[6], double* eval, double evec[3]) {
  double scale = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) scale = fmax(scale, fabs(cov[k]));
  if (scale <= DBL_MIN) scale = 1.0;
  double m[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) m[k] = cov[k] / scale;
  double r[3];
  roots3(m, r);
  *eval = r[0] * scale;
  const double a00 = m[0] - r[0], a11 = m[3] - r[0], a22 = m[5] - r[0];
  const double r0[3] = {a00, m[1], m[2]}, r1[3] = {m[1], a11, m[4]}, r2[3] = {m[2], m[4], a22};
  const double v1[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
  const double v2[3] = {r0[1] * r2[2] - r0[2] * r2[1], r0[2] * r2[0] - r0[0] * r2[2], r0[0] * r2[1] - r0[1] * r2[0]};
  const double v3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
  const double l1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
  const double l2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  const double l3 = v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2];
  const double* v;
  double l;
  if (l1 >= l2 && l1 >= l3) { v = v1; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { v = v2; l = l2; }
  else { v = v3; l = l3; }
  const double s = sqrt(l);
  evec[0] = v[0] / s;
  evec[1] = v[1] / s;
  evec[2] = v[2] / s;
}

}  // namespace pgp
