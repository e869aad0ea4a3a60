// csrc/icp_solve.h -- the device functions every ICP kernel shares (icp.hip, tricp_states.hip): the placement of a
// point by one row of a column-major 4x4, rounded operation by operation, and Horn's closed-form rigid update from the
// float64 sums of an iteration.  One copy, so that the forms that are compared with each other cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>

namespace pgp {
namespace {

__device__ __forceinline__ float row_xf(float a, float b, float c, float t, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), t);
}

// cyclic Jacobi on a symmetric 4x4 (double); returns the eigenvector of the largest eigenvalue.
// The rotation planes (p, r) and the inner index are fully unrolled, so every A[..][..] / V[..][..] has
// compile-time indices and the two matrices live in VGPRs (run-time indexed private arrays would go
// to scratch, cdna_hip_programming.md rule 20; round 1 kept them in LDS, where the single working
// lane paid an LDS round trip per element: ~60 of the 96 us of an icp_refine launch).  Same
// operations in the same order as before (and as oracle/pgp_oracle.c jacobi_eig4).
__device__ void largest_eigvec4(double (&A)[4][4], double q[4]) {
  double V[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) V[p][r] = p == r ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) off += A[p][r] * A[p][r];
    if (off < 1e-300) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double apr = A[p][r];
        if (apr != 0.0) {
          const double theta = (A[r][r] - A[p][p]) / (2.0 * apr);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // A <- A J
            const double akp = A[k][p], akr = A[k][r];
            A[k][p] = c * akp - sn * akr;
            A[k][r] = sn * akp + c * akr;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // A <- J^T A
            const double apk = A[p][k], ark = A[r][k];
            A[p][k] = c * apk - sn * ark;
            A[r][k] = sn * apk + c * ark;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double vkp = V[k][p], vkr = V[k][r];
            V[k][p] = c * vkp - sn * vkr;
            V[k][r] = sn * vkp + c * vkr;
          }
        }
      }
  }
  int best = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const double ak = k == 1 ? A[1][1] : (k == 2 ? A[2][2] : A[3][3]);
    const double ab = best == 0 ? A[0][0] : (best == 1 ? A[1][1] : (best == 2 ? A[2][2] : A[3][3]));
    if (ak > ab) best = k;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = best == 0 ? V[k][0] : (best == 1 ? V[k][1] : (best == 2 ? V[k][2] : V[k][3]));
}

// The same eigenvector without iterating over rotations: Horn's N is symmetric and traceless, so its
// characteristic polynomial is l^4 + c2 l^2 + c1 l + c0 with c2 = -tr(N^2)/2, c1 = -tr(N^3)/3, c0 = det N
// (Newton's identities); it is convex and increasing beyond its largest root, so Newton's iteration from
// the Gershgorin bound descends monotonically onto that root (Horn 1987 section 4; Theobald 2005), and
// every non-zero column of adj(N - l I) is the eigenvector.  ~400 f64 operations against ~50 Jacobi
// rotations of four divisions / square roots each: 27 us -> 2 us of ONE lane per ICP iteration
// (DESIGN.md).  Returns false -- the caller falls back to the Jacobi sweeps -- when the largest
// eigenvalue is (nearly) double: the adjugate then vanishes and the rotation is not unique.
__device__ __forceinline__ double det3(double a, double b, double c, double d, double e, double f, double g, double h,
                                       double i) {
  return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}
__device__ bool largest_eigvec4_direct(const double (&N)[4][4], double q[4]) {
  const double a00 = N[0][0], a01 = N[0][1], a02 = N[0][2], a03 = N[0][3], a11 = N[1][1], a12 = N[1][2], a13 = N[1][3],
               a22 = N[2][2], a23 = N[2][3], a33 = N[3][3];
  // N^2 (symmetric)
  const double m00 = a00 * a00 + a01 * a01 + a02 * a02 + a03 * a03, m01 = a00 * a01 + a01 * a11 + a02 * a12 + a03 * a13,
               m02 = a00 * a02 + a01 * a12 + a02 * a22 + a03 * a23, m03 = a00 * a03 + a01 * a13 + a02 * a23 + a03 * a33,
               m11 = a01 * a01 + a11 * a11 + a12 * a12 + a13 * a13, m12 = a01 * a02 + a11 * a12 + a12 * a22 + a13 * a23,
               m13 = a01 * a03 + a11 * a13 + a12 * a23 + a13 * a33, m22 = a02 * a02 + a12 * a12 + a22 * a22 + a23 * a23,
               m23 = a02 * a03 + a12 * a13 + a22 * a23 + a23 * a33, m33 = a03 * a03 + a13 * a13 + a23 * a23 + a33 * a33;
  const double p2 = m00 + m11 + m22 + m33;
  const double p3 = (m00 * a00 + m11 * a11 + m22 * a22 + m33 * a33) +
                    2.0 * (m01 * a01 + m02 * a02 + m03 * a03 + m12 * a12 + m13 * a13 + m23 * a23);
  const double det = a00 * det3(a11, a12, a13, a12, a22, a23, a13, a23, a33) - a01 * det3(a01, a12, a13, a02, a22, a23, a03, a23, a33) +
                     a02 * det3(a01, a11, a13, a02, a12, a23, a03, a13, a33) - a03 * det3(a01, a11, a12, a02, a12, a22, a03, a13, a23);
  const double c2 = -0.5 * p2, c1 = -p3 / 3.0, c0 = det;
  double lam = fmax(fmax(fabs(a00) + fabs(a01) + fabs(a02) + fabs(a03), fabs(a01) + fabs(a11) + fabs(a12) + fabs(a13)),
                    fmax(fabs(a02) + fabs(a12) + fabs(a22) + fabs(a23), fabs(a03) + fabs(a13) + fabs(a23) + fabs(a33)));
  if (!(lam > 0.0)) return false;
  for (int it = 0; it < 64; ++it) {
    const double l2 = lam * lam;
    const double P = (l2 + c2) * l2 + c1 * lam + c0, dP = (4.0 * l2 + 2.0 * c2) * lam + c1;
    if (!(dP > 0.0)) break;
    const double nl = lam - P / dP;
    if (!(nl < lam)) break;   // monotone from above: no further descent = converged to the rounding of P
    lam = nl;
  }
  const double b00 = a00 - lam, b11 = a11 - lam, b22 = a22 - lam, b33 = a33 - lam;
  // adj(B), B = N - lam I symmetric: cofactor(i, j) = (-1)^(i+j) det(B without row i and column j)
  const double k00 = det3(b11, a12, a13, a12, b22, a23, a13, a23, b33), k11 = det3(b00, a02, a03, a02, b22, a23, a03, a23, b33),
               k22 = det3(b00, a01, a03, a01, b11, a13, a03, a13, b33), k33 = det3(b00, a01, a02, a01, b11, a12, a02, a12, b22);
  const double k01 = -det3(a01, a12, a13, a02, b22, a23, a03, a23, b33), k02 = det3(a01, b11, a13, a02, a12, a23, a03, a13, b33),
               k03 = -det3(a01, b11, a12, a02, a12, b22, a03, a13, a23), k12 = -det3(b00, a01, a03, a02, a12, a23, a03, a13, b33),
               k13 = det3(b00, a01, a02, a02, a12, b22, a03, a13, a23), k23 = -det3(b00, a01, a02, a01, b11, a12, a03, a13, a23);
  // adj(B) = kappa v v^T: the column with the largest diagonal entry is the best conditioned one
  const double d0 = fabs(k00), d1 = fabs(k11), d2 = fabs(k22), d3 = fabs(k33);
  const double dm = fmax(fmax(d0, d1), fmax(d2, d3));
  if (!(dm > 1e-6 * lam * lam * lam)) return false;
  if (d0 == dm) { q[0] = k00; q[1] = k01; q[2] = k02; q[3] = k03; }
  else if (d1 == dm) { q[0] = k01; q[1] = k11; q[2] = k12; q[3] = k13; }
  else if (d2 == dm) { q[0] = k02; q[1] = k12; q[2] = k22; q[3] = k23; }
  else { q[0] = k03; q[1] = k13; q[2] = k23; q[3] = k33; }
  return true;
}

// Horn's closed form from the f64 sums over the selected pairs:
// red = {n, sx,sy,sz, mx,my,mz, Sxx,Sxy,Sxz, Syx,Syy,Syz, Szx,Szy,Szz}  (S_ab = sum s_a m_b)
__device__ __attribute__((noinline)) void solve_rigid(const double* red, float* G) {
  double n = red[0];
  if (!(n >= 1.0)) return;  // nothing selected: keep G
  double sb[3] = {red[1] / n, red[2] / n, red[3] / n}, mb[3] = {red[4] / n, red[5] / n, red[6] / n};
  const double Sxx = red[7] - n * sb[0] * mb[0], Sxy = red[8] - n * sb[0] * mb[1], Sxz = red[9] - n * sb[0] * mb[2];
  const double Syx = red[10] - n * sb[1] * mb[0], Syy = red[11] - n * sb[1] * mb[1], Syz = red[12] - n * sb[1] * mb[2];
  const double Szx = red[13] - n * sb[2] * mb[0], Szy = red[14] - n * sb[2] * mb[1], Szz = red[15] - n * sb[2] * mb[2];
  double N[4][4];
  N[0][0] = Sxx + Syy + Szz; N[0][1] = Syz - Szy;       N[0][2] = Szx - Sxz;        N[0][3] = Sxy - Syx;
  N[1][0] = Syz - Szy;       N[1][1] = Sxx - Syy - Szz; N[1][2] = Sxy + Syx;        N[1][3] = Szx + Sxz;
  N[2][0] = Szx - Sxz;       N[2][1] = Sxy + Syx;       N[2][2] = -Sxx + Syy - Szz; N[2][3] = Syz + Szy;
  N[3][0] = Sxy - Syx;       N[3][1] = Szx + Sxz;       N[3][2] = Syz + Szy;        N[3][3] = -Sxx - Syy + Szz;
  double q[4];
  if (!largest_eigvec4_direct(N, q)) largest_eigvec4(N, q);
  double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!(nq > 0.0)) return;
  double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
  double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                    {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                    {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double t = mb[r] - (R[r][0] * sb[0] + R[r][1] * sb[1] + R[r][2] * sb[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) G[4 * c + r] = (float)R[r][c];
    G[12 + r] = (float)t;
  }
  G[3] = G[7] = G[11] = 0.f;
  G[15] = 1.f;
}

}  // namespace
}  // namespace pgp
