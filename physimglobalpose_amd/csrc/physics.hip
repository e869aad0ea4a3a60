// csrc/physics.hip -- physics settling of MCTS child states: UCTState::correctPhysics on the device.
//
// The reference (PPE/hypothesis_verification/mcts/UCTState.cpp:208-270, physics_reasoning/PhySim.cpp) drops the newest
// object into a Bullet 2.86 world among the earlier objects (mass 0) and the table box, runs 60 x stepSimulation(1/60)
// and reads the pose back.  Bullet is not matched bit for bit; this file runs the rules below EXACTLY, and
// tests/_physics_restate.py (steps 1 .. 6), tests/_physics_edges_restate.py (with step 3e) and
// tests/_physics_sat_restate.py (with step 3p) restate them in numpy float32, term by term.  Every operation is float32, rounded
// separately (-ffp-contract=off), sums left to right as written; sqrt(x) = (float)sqrt((double)x) and a / b = __fdiv_rn,
// both correctly rounded.  One dynamic body D per state; the others (the table first, then the statics in the caller's
// order) are static S.  Mass cancels: impulses are per unit mass, 1/m = 1.
//
// Shapes (pgp_physics_add_shape): hull vertices v and planes (n, d) (n . x <= d inside) in the body frame, margin m,
// radius r (bounding sphere about the body origin), unit-mass inertia diagonal I (see include/pgp.h), and the hull's
// edges as rows (v0, v1, f0, f1): two vertices shared by two triangles of the hull whose merged planes f0 < f1 differ
// (a side between coplanar triangles that merged into one plane is no edge), v0 < v1, rows ascending by (v0, v1).
// Poses: W_D = cam . T (4 x 4 column-major products, element (i, j) = ((C_i0 T_0j + C_i1 T_1j) + C_i2 T_2j) + C_i3 T_3j),
// W_S = cam . T_S likewise (cam NULL: W = T); the table's R, t are the rows of tableParams.  R_D -> q by Shepperd's
// method, then q /= |q| (quat_from_R); R(q) is Bullet's setRotation matrix (R_from_q).  x = W_D's translation.
// State at rest: v = w = 0.  c_lin = (float)pow(1 - (double)damping, (double)dt) on the host, likewise c_ang.
//
// One step:
//  1. v = (v + dt g) * c_lin, w = w * c_ang; L = |w|; if L dt > pi/2 (float): w = w * ((pi/2) / dt / L)
//     (w_max = (pi/2) / dt formed on the host in float).
//  2. R = R(q), Iw = R diag(1/I) R^T with Iw_ij = ((R_i0 ix) R_j0 + (R_i1 iy) R_j1) + (R_i2 iz) R_j2, ix = 1 / I_x.
//     World vertices of D: p = R v + x, p_i = ((R_i0 v_x + R_i1 v_y) + R_i2 v_z) + x_i.
//  3. Contacts, per pair (D, S), S in order: skipped when |t_S - x|^2 > ((r_D + r_S) + (m_D + m_S))^2 (part of the
//     rule).  With m = m_D + m_S, candidates are numbered D's vertices first, then S's:
//       D vertex p (world): u = p - t_S, p_S = R_S^T u (p_S,i = (R_0i u_x + R_1i u_y) + R_2i u_z); s_f = ((n_x p_x +
//       n_y p_y) + n_z p_z) - d over S's planes in order; a candidate when every s_f < m; the face is the first
//       maximal s_f (the least penetrated); normal R_S n_f; point p; depth = max s_f - m.
//       S vertex s: p = R_S s + t_S (world), p_D = R^T (p - x), s_f over D's planes; normal -(R n_f); point p.
//     The plane loop stops at the first s_f >= m (exact: such a vertex is no candidate).
//  3e. Edge-edge candidates of the pair, only with pgp_physics_set_edge_contacts on (reach: its second argument):
//     Active edges: an edge of D is active unless one plane of S has BOTH its end points at s_f >= m, the end points
//     taken in S's frame with the s_f expression above; an edge of S likewise against D's planes (its end points
//     p = R_S s + t_S, p_D = R^T (p - x)).  Active edges keep their ascending edge index.
//     Pairs (active D edge a0 a1, active S edge b0 b1, world points), ascending by (D edge, S edge):
//       d1 = a1 - a0, d2 = b1 - b0, r = a0 - b0; a = d1 . d1, e = d2 . d2, b = d1 . d2, c = d1 . r, f = d2 . r (each
//       (x x + y y) + z z); den = a e - b b; rejected unless den > 1e-6f (a e) (parallel edges);
//       s = (b f - c e) / den, t = (a f - b c) / den; rejected unless 0 < s < 1 and 0 < t < 1 (end points stay with
//       the vertex test); c_D = a0 + s d1, c_S = b0 + t d2 (per component a0_i + s d1_i); g = c_D - c_S; rejected
//       when |g|^2 > reach reach (a far-side pair of two overlapping flat bodies would be the deepest candidate);
//       rejected unless every s_f of c_D over S's planes is < m (u = c_D - t_S, as for a D vertex) and every s_f of
//       c_S over D's planes is < m (u = c_S - x, as for an S vertex);
//       n = (d1 x d2) / |d1 x d2| (each component divided by L = sqrt(|d1 x d2|^2));
//       o_S = R_S (n_f0 + n_f1) of the S edge's planes, o_D = R (n_f0 + n_f1) of the D edge's (sums per component,
//       then (R_i0 q_x + R_i1 q_y) + R_i2 q_z); n = -n when n . o_S < 0; rejected unless then n . o_S > 0 and
//       n . o_D < 0 (n leaves S and enters D);
//       candidate: point c_D, normal n, depth = (n . g) - m.
//     Edge candidates are numbered after D's and S's vertex candidates, in pair order; a pair has room for 512
//     candidates in all, and edge candidates past it are dropped, in pair order.
//  3p. Polyhedral contacts, only with pgp_physics_set_polyhedral_contacts on (face_bias: its second argument); they
//     replace 3 and 3e, whatever the edge switch says; the sphere rule of 3 stays.  Shapes carry, per plane, the loop
//     of its vertices, counter-clockwise seen from outside, from its lowest vertex index (tests/_physics_sat_restate.py
//     restates the loops and this step).  Per pair (D, S), m = m_D + m_S, s_f the expression of 3:
//     Face queries: sep_S(f) = min s_f over D's vertices (taken into S's frame as in 3) for each plane f of S,
//       sep_D(f) = min s_f over S's vertices (p = R_S s + t_S, p_D = R^T (p - x)) for each plane f of D; best_S, best_D
//       = the first maximal sep; the vertex of a plane = the first that attains its sep.  best_S >= m or best_D >= m:
//       no contacts.
//     Edge query, pairs (a of D: a0 a1, planes f0 f1; b of S: b0 b1) ascending by (D edge, S edge), world frame:
//       A = R n_f0, B = R n_f1 of a; C = -(R_S n_f0), E = -(R_S n_f1) of b (each (R_i0 n_x + R_i1 n_y) + R_i2 n_z);
//       the pair counts only when the arcs AB and CE cross on the Gauss map (then a and b span a face of the Minkowski
//       difference): with U = B x A, V = E x C: (C . U) (E . U) < 0 and (A . V) (B . V) < 0 and (C . U) (B . V) > 0;
//       d1, d2, a, e, b, den and the parallel rejection den > 1e-6f (a e) of 3e; n = (d1 x d2) / |d1 x d2|, o_S, o_D,
//       the flip and the rejection unless n . o_S > 0 and n . o_D < 0 of 3e; sep_E = n . r, r = a0 - b0.
//       best_E = the first maximal sep_E (a NaN is no maximum); best_E >= m: no contacts.
//     Choice: an edge contact when a pair counted and best_E > max(best_S, best_D) + face_bias; else a face contact,
//       the reference body S when best_S >= best_D, else D.  (A face gives a manifold, an edge one point: the bias
//       keeps nearly equal penetrations from flickering between them.)
//     Edge contact, of the pair of best_E: c = d1 . r, f = d2 . r, s = (b f - c e) / den clamped to [0, 1] (t does not
//       enter: the point is D's); one candidate: point c_D = a0 + s d1, normal n, depth best_E - m.
//     Face contact: f* the reference plane, N = R_ref n_f* (world).  Incident face g: the plane of the other body with
//       the first least N . (R_inc n_g).  Polygon: g's loop in world coordinates (D: the step's world vertices; S:
//       R_S s + t_S).  For each side k of f*'s loop in loop order, u = world vertex k, w = the next one (cyclic),
//       K = (w - u) x N, side(p) = K . (p - u); p is kept when side(p) <= 0.  One pass visits the polygon's edges a -> b
//       (b the next point, cyclic) in order and emits a when a is kept, then, when exactly one of a, b is kept, the
//       crossing a + t (b - a), t = side(a) / (side(a) - side(b)), per component a_i + t (b_i - a_i)
//       (Sutherland-Hodgman).  A polygon holds at most 512 points: later ones are dropped in output order (two loops
//       of at most 256 vertices stay below it unless rounding breaks convexity).
//       Candidates: the clipped polygon's points in output order whose s = s_f*(p) (p into the reference body's frame
//       as in 3) is < m: point p, depth s - m, normal N when the reference is S, -N (per component) when it is D.
//       An empty polygon: one candidate, the incident body's vertex of f* (above), depth best - m, the same normal.
//     Limits: one point for an edge-edge contact; no persistent manifold, no warm start; no closest features of
//     separated hulls (a pair farther apart than m has no contacts); the edge query visits E_D x E_S pairs.
//  4. Manifold reduction, when a pair has more than 4 candidates (else all of them, in candidate order): c1 = the
//     least depth; c2 = max |p - p1|^2; c3 = max |(p - p1) x (p - p2)|^2; c4 = max of the sum
//     (|(p - p1) x (p - p2)|^2 + |(p - p2) x (p - p3)|^2) + |(p - p3) x (p - p1)|^2; each among the candidates not
//     yet picked, ties to the lowest candidate number; |a|^2 = (a_x a_x + a_y a_y) + a_z a_z, a x b written out
//     (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x).  Contacts are kept as c1, c2, c3, c4, pairs in order.
//  5. Sequential impulses, rows built at the step's pose: for contact (p, n, depth), r = p - x; for each row
//     direction u (n, then t1, t2 = btPlaneSpace1(n)): ca = r x u, aa = Iw ca (aa_i = (Iw_i0 ca_x + Iw_i1 ca_y) +
//     Iw_i2 ca_z), j = 1 / (1 + u . (aa x r)), lambda = 0.  Normal target tgt = max(0, ((-depth) beta) / dt),
//     friction target 0.  Each of `iterations` sweeps visits every normal row in contact order, then per contact its
//     t1 and t2 rows:  vn = (u . v) + (ca . w);  l = lambda + (tgt - vn) j;  normal: l = max(l, 0); friction:
//     clamped to [-mu lambda_n, mu lambda_n] (lambda_n the contact's current normal impulse); dl = l - lambda;
//     lambda = l; v = v + u dl; w = w + aa dl.  No warm start between steps; statics do not move.
//  6. x = x + dt v; q = q + (dt / 2) o with o = (w, 0) (x) q, o_x = (w_x q_w + w_y q_z) - w_z q_y, o_y = (w_y q_w +
//     w_z q_x) - w_x q_z, o_z = (w_z q_w + w_x q_y) - w_y q_x, o_w = -((w_x q_x + w_y q_y) + w_z q_z), then
//     q = q / |q|.  (Bullet integrates with the exponential map; this first-order update needs only + - x / sqrt.)
// Out: W = [R(q) | x], T_out = cam^-1 . W (cam^-1 the rigid inverse formed on the host in float: R^T,
// -(((R_0i t_0 + R_1i t_1) + R_2i t_2))), or W without cam.  steps == 0: T_out = T, bit for bit.
// Contacts are vertex-face, plus edge-edge behind the switch; no persistent manifold, no split impulse, no
// restitution.  Limits of 3e: a body thinner than reach can pick up an edge pair of its far side; an overlap deeper
// than reach falls back to vertex-face contacts; it is still not GJK/EPA.  Step 3p has no reach; its limits stand with it.
//
// Kernel: one workgroup of 256 threads per state, all steps in one launch.  D's hull (body and world frame) and
// planes sit in LDS; candidates are tested one vertex per thread and compacted in vertex order with a ballot and
// a prefix; the reduction is a block arg-max with lowest-index ties; the impulse loop is a chain of dependent row
// updates and runs on one lane.  The planes of each static body are staged into LDS per pair and step (the plane
// loop of a vertex is a chain of dependent loads: from L2 it cost ~8x more with 256-vertex hulls); its vertices
// are read from the arena (it stays in L2) and transformed on the fly.  Step 3e (settle_kernel<true> only): one
// edge per thread and pass of 256 for the activity test, compacted like the candidates into 16-bit indices in LDS;
// then one edge pair per thread and pass, compacted behind the vertex candidates; every loop is bounded by the edge
// counts.  Workgroups never talk to each other, so a state's result is independent of its batch.
// Step 3p (settle_poly_kernel, a sibling with the same steps around it): face queries one plane per thread over the
// other body's vertices, staged in LDS in the planes' frame, then a block arg-max; D's edges (world end points and
// normals) are staged per step and S's per pair, 36 KB each at the cap, and the edge query runs one pair per thread and
// pass; the clipping runs one side of the reference loop per pass and one polygon edge per thread, the 0 .. 2 points of
// each compacted in order by a block scan from one LDS polygon into the other.  Every loop is bounded by vertex, plane,
// edge or loop counts.  131 KB of LDS: one workgroup per CU.
#include <algorithm>
#include <array>
#include <cfloat>
#include <climits>
#include <cmath>
#include <map>
#include <set>
#include <utility>

#include "pgp_internal.h"
#include "wave.h"

using namespace pgp;

namespace {

constexpr int PT = 256;                                     // threads per state
constexpr int MAXV = PGP_PHYSICS_MAX_VERTICES;
constexpr int MAXP = 2 * MAXV;                              // plane capacity of a shape (a hull has <= 2V - 4)
constexpr int MAXE = PGP_PHYSICS_MAX_EDGES;                 // edge capacity of a shape (a hull has <= 3V - 6)
constexpr int MAXB = 1 + PGP_PHYSICS_MAX_STATICS;           // bodies besides D
constexpr int MAXC = PGP_PHYSICS_MAX_CONTACTS;
constexpr float HALF_PI_F = 1.57079637f;
constexpr float SQRT12_F = 0.707106781f;
constexpr int TRACE_STATE = PHYS_TRACE_STATE, TRACE_CONTACT = PHYS_TRACE_CONTACT;


__device__ __forceinline__ float fsq(float x) { return (float)__dsqrt_rn((double)x); }
__device__ __forceinline__ float fdv(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float norm2_3(float x, float y, float z) { return (x * x + y * y) + z * z; }

// column-major 4x4 product A . B
__device__ void mat4_mul(const float* A, const float* B, float* O) {
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 4; ++i)
      O[j * 4 + i] = ((A[i] * B[j * 4] + A[4 + i] * B[j * 4 + 1]) + A[8 + i] * B[j * 4 + 2]) + A[12 + i] * B[j * 4 + 3];
}

// Shepperd's method on R (row-major), then q /= |q|; q = (x, y, z, w)
__device__ void quat_from_R(const float* R, float* q) {
  const float r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
  const float tr = (r00 + r11) + r22;
  float x, y, z, w;
  if (tr > 0.f) {
    const float s = fsq(tr + 1.f) * 2.f;
    w = 0.25f * s; x = fdv(r21 - r12, s); y = fdv(r02 - r20, s); z = fdv(r10 - r01, s);
  } else if (r00 > r11 && r00 > r22) {
    const float s = fsq(((1.f + r00) - r11) - r22) * 2.f;
    w = fdv(r21 - r12, s); x = 0.25f * s; y = fdv(r01 + r10, s); z = fdv(r02 + r20, s);
  } else if (r11 > r22) {
    const float s = fsq(((1.f + r11) - r00) - r22) * 2.f;
    w = fdv(r02 - r20, s); x = fdv(r01 + r10, s); y = 0.25f * s; z = fdv(r12 + r21, s);
  } else {
    const float s = fsq(((1.f + r22) - r00) - r11) * 2.f;
    w = fdv(r10 - r01, s); x = fdv(r02 + r20, s); y = fdv(r12 + r21, s); z = 0.25f * s;
  }
  const float n = fsq(((x * x + y * y) + z * z) + w * w);
  q[0] = fdv(x, n); q[1] = fdv(y, n); q[2] = fdv(z, n); q[3] = fdv(w, n);
}

// btMatrix3x3::setRotation
__device__ void R_from_q(const float* q, float* R) {
  const float x = q[0], y = q[1], z = q[2], w = q[3];
  const float d = ((x * x + y * y) + z * z) + w * w;
  const float s = fdv(2.f, d);
  const float xs = x * s, ys = y * s, zs = z * s;
  const float wx = w * xs, wy = w * ys, wz = w * zs;
  const float xx = x * xs, xy = x * ys, xz = x * zs;
  const float yy = y * ys, yz = y * zs, zz = z * zs;
  R[0] = 1.f - (yy + zz); R[1] = xy - wz;         R[2] = xz + wy;
  R[3] = xy + wz;         R[4] = 1.f - (xx + zz); R[5] = yz - wx;
  R[6] = xz - wy;         R[7] = yz + wx;         R[8] = 1.f - (xx + yy);
}

// one row of the sequential impulses: u, ca, aa, j, tgt, lambda; bounds lo / hi
struct Row {
  float u[3], ca[3], aa[3];
  float j, tgt, lambda;
};

__device__ void row_build(Row& rw, const float* r, const float* u, const float* Iw, float tgt) {
  rw.u[0] = u[0]; rw.u[1] = u[1]; rw.u[2] = u[2];
  cross3(r, u, rw.ca);
  for (int i = 0; i < 3; ++i) rw.aa[i] = (Iw[3 * i] * rw.ca[0] + Iw[3 * i + 1] * rw.ca[1]) + Iw[3 * i + 2] * rw.ca[2];
  float vec[3];
  cross3(rw.aa, r, vec);
  rw.j = fdv(1.f, 1.f + dot3(u, vec));
  rw.tgt = tgt;
  rw.lambda = 0.f;
}

__device__ __forceinline__ void row_solve(Row& rw, float lo, float hi, float* v, float* w) {
  const float vn = dot3(rw.u, v) + dot3(rw.ca, w);
  float l = rw.lambda + (rw.tgt - vn) * rw.j;
  if (l < lo) l = lo;
  if (l > hi) l = hi;
  const float dl = l - rw.lambda;
  rw.lambda = l;
  for (int i = 0; i < 3; ++i) v[i] = v[i] + rw.u[i] * dl;
  for (int i = 0; i < 3; ++i) w[i] = w[i] + rw.aa[i] * dl;
}

// btPlaneSpace1
__device__ void plane_space(const float* n, float* p, float* q) {
  if (fabsf(n[2]) > SQRT12_F) {
    const float a = n[1] * n[1] + n[2] * n[2];
    const float k = fdv(1.f, fsq(a));
    p[0] = 0.f; p[1] = -n[2] * k; p[2] = n[1] * k;
    q[0] = a * k; q[1] = -n[0] * p[2]; q[2] = n[0] * p[1];
  } else {
    const float a = n[0] * n[0] + n[1] * n[1];
    const float k = fdv(1.f, fsq(a));
    p[0] = -n[1] * k; p[1] = n[0] * k; p[2] = 0.f;
    q[0] = -n[2] * p[1]; q[1] = n[2] * p[0]; q[2] = a * k;
  }
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// EDGES = false is the vertex-face kernel: step 3e is compiled out, not branched over, and PhysShape, which this kernel
// stages whole, keeps its 40 bytes (the edge slices live beside it in PhysEdgeSlice): that instantiation is the kernel
// of before, instruction for instruction and at the same offsets.  It matters: the same loops moved by 8 .. 40 bytes
// ran 4-9 % slower or faster, row by row (DESIGN.md section 4 has the figures of both instantiations and of the moves)
template <bool EDGES>
__global__ void __launch_bounds__(PT) settle_kernel(PhysParams P, const PhysShape* __restrict__ shapes,
                                                    const float4* __restrict__ verts, const float4* __restrict__ planes,
                                                    const int* __restrict__ dyn_shape, const float* T,
                                                    const int* __restrict__ static_off, const int* __restrict__ static_shape,
                                                    const float* __restrict__ static_T, float* T_out,
                                                    pgp_physics_info* __restrict__ info, float* __restrict__ tr_state,
                                                    float* __restrict__ tr_contacts, int* __restrict__ tr_n,
                                                    const PhysEdgeSlice* __restrict__ eslice, const int4* __restrict__ edges,
                                                    float reach) {
  __shared__ float4 s_dv[MAXV];        // D's hull, body frame
  __shared__ float4 s_dw[MAXV];        // D's hull, world frame of the step
  __shared__ float4 s_dp[MAXP];        // D's planes, body frame
  __shared__ float4 s_sp[MAXP];        // the planes of the pair's static body S, body frame
  __shared__ float4 s_cp[2 * PT];      // candidates: point (xyz), depth (w)
  __shared__ float4 s_cn[2 * PT];      // candidates: normal
  __shared__ float s_body[MAXB][12];   // R (row-major) | t of the table and the statics, world frame
  __shared__ PhysShape s_sh[MAXB + 1]; // [0] = D, [1 + j] = body j
  __shared__ PhysEdgeSlice s_er[EDGES ? MAXB + 1 : 1];   // their edge slices, settle_kernel<true> only
  __shared__ float4 s_ctp[MAXC], s_ctn[MAXC];
  __shared__ Row s_rows[3 * MAXC];
  __shared__ float s_x[3], s_q[4], s_v[3], s_w[3], s_R[9], s_Iw[9], s_Tin[16];
  __shared__ int s_ok, s_nb, s_nct, s_wc[8], s_pick[4], s_ri[4];
  __shared__ float s_rv[4];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int st = blockIdx.x;
  if (st >= P.n_states) return;

  if (tid == 0) {
    int ok = 1;
    const int dyn = dyn_shape[st];
    const int o0 = static_off[st], o1 = static_off[st + 1];
    if (dyn < 0 || dyn >= P.n_shapes || o0 < 0 || o1 < o0 || o1 - o0 > PGP_PHYSICS_MAX_STATICS) ok = 0;
    if (ok)
      for (int k = o0; k < o1; ++k)
        if (static_shape[k] < 0 || static_shape[k] >= P.n_shapes) ok = 0;
    for (int k = 0; k < 16; ++k) {
      s_Tin[k] = T[(size_t)st * 16 + k];
      if (!isfinite(s_Tin[k])) ok = 0;
    }
    if (ok) {
      s_sh[0] = shapes[dyn];
      s_sh[1] = shapes[0];
      if constexpr (EDGES) {
        s_er[0] = eslice[dyn];
        s_er[1] = eslice[0];
      }
      for (int i = 0; i < 3; ++i) {
        for (int c = 0; c < 3; ++c) s_body[0][3 * i + c] = P.table[4 * i + c];
        s_body[0][9 + i] = P.table[4 * i + 3];
      }
      for (int k = o0; k < o1; ++k) {
        const int b = 1 + (k - o0);
        s_sh[1 + b] = shapes[static_shape[k]];
        if constexpr (EDGES) s_er[1 + b] = eslice[static_shape[k]];
        float Ts[16], W[16];
        for (int e = 0; e < 16; ++e) Ts[e] = static_T[(size_t)k * 16 + e];
        if (P.has_cam) mat4_mul(P.cam, Ts, W);
        else
          for (int e = 0; e < 16; ++e) W[e] = Ts[e];
        for (int i = 0; i < 3; ++i) {
          for (int c = 0; c < 3; ++c) s_body[b][3 * i + c] = W[c * 4 + i];
          s_body[b][9 + i] = W[12 + i];
        }
      }
      s_nb = 1 + (o1 - o0);
      float W[16];
      if (P.has_cam) mat4_mul(P.cam, s_Tin, W);
      else
        for (int e = 0; e < 16; ++e) W[e] = s_Tin[e];
      float R[9];
      for (int i = 0; i < 3; ++i)
        for (int c = 0; c < 3; ++c) R[3 * i + c] = W[c * 4 + i];
      quat_from_R(R, s_q);
      for (int i = 0; i < 3; ++i) { s_x[i] = W[12 + i]; s_v[i] = 0.f; s_w[i] = 0.f; }
    }
    s_ok = ok;
  }
  __syncthreads();
  if (!s_ok || P.steps == 0) {
    if (tid < 16) T_out[(size_t)st * 16 + tid] = s_ok ? s_Tin[tid] : __int_as_float(0x7fc00000);
    if (tid == 0 && info) {
      pgp_physics_info inf;
      inf.n_contacts = s_ok ? 0 : -1;
      inf.min_depth = 0.f; inf.lin_speed = 0.f; inf.ang_speed = 0.f;
      info[st] = inf;
    }
    return;
  }
  const PhysShape D = s_sh[0];
  for (int i = tid; i < D.n_vert; i += PT) s_dv[i] = verts[D.vert_off + i];
  for (int f = tid; f < D.n_plane; f += PT) s_dp[f] = planes[D.plane_off + f];
  const float inv_i[3] = {fdv(1.f, D.inertia[0]), fdv(1.f, D.inertia[1]), fdv(1.f, D.inertia[2])};
  const int nb = s_nb;

  for (int step = 0; step < P.steps; ++step) {
    // 1-2: velocities, damping, clamp; R, Iw
    if (tid == 0) {
      float* v = s_v; float* w = s_w;
      for (int i = 0; i < 3; ++i) v[i] = (v[i] + P.dt * P.g[i]) * P.lin_c;
      for (int i = 0; i < 3; ++i) w[i] = w[i] * P.ang_c;
      const float L = fsq(norm2_3(w[0], w[1], w[2]));
      if (L * P.dt > HALF_PI_F) {
        const float sc = fdv(P.w_max, L);
        for (int i = 0; i < 3; ++i) w[i] = w[i] * sc;
      }
      R_from_q(s_q, s_R);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          s_Iw[3 * i + j] = ((s_R[3 * i] * inv_i[0]) * s_R[3 * j] + (s_R[3 * i + 1] * inv_i[1]) * s_R[3 * j + 1]) +
                            (s_R[3 * i + 2] * inv_i[2]) * s_R[3 * j + 2];
      s_nct = 0;
    }
    __syncthreads();
    float R[9], x[3];
    for (int k = 0; k < 9; ++k) R[k] = s_R[k];
    for (int k = 0; k < 3; ++k) x[k] = s_x[k];
    for (int i = tid; i < D.n_vert; i += PT) {
      const float4 a = s_dv[i];
      s_dw[i] = make_float4(((R[0] * a.x + R[1] * a.y) + R[2] * a.z) + x[0], ((R[3] * a.x + R[4] * a.y) + R[5] * a.z) + x[1],
                            ((R[6] * a.x + R[7] * a.y) + R[8] * a.z) + x[2], 0.f);
    }
    __syncthreads();

    // 3-4: contacts pair by pair
    for (int b = 0; b < nb; ++b) {
      const PhysShape S = s_sh[1 + b];
      const float* B = s_body[b];
      const float m = D.margin + S.margin;
      {
        const float dx = B[9] - x[0], dy = B[10] - x[1], dz = B[11] - x[2];
        const float rr = (D.radius + S.radius) + m;
        if (norm2_3(dx, dy, dz) > rr * rr) continue;   // uniform over the block
      }
      for (int f = tid; f < S.n_plane; f += PT) s_sp[f] = planes[S.plane_off + f];
      __syncthreads();
      const int total = D.n_vert + S.n_vert;
      float4 cp[2], cn[2];
      bool fl[2];
      for (int h = 0; h < 2; ++h) {
        const int k = h * PT + tid;
        fl[h] = false;
        if (k >= total) continue;
        float p[3], ploc[3];
        const float4* pl;
        int npl;
        float sgn;
        const float* Rn;   // rotation of the face normals into the world
        if (k < D.n_vert) {
          const float4 a = s_dw[k];
          p[0] = a.x; p[1] = a.y; p[2] = a.z;
          const float u[3] = {p[0] - B[9], p[1] - B[10], p[2] - B[11]};
          for (int i = 0; i < 3; ++i) ploc[i] = (B[i] * u[0] + B[3 + i] * u[1]) + B[6 + i] * u[2];
          pl = s_sp; npl = S.n_plane; sgn = 1.f; Rn = B;
        } else {
          const float4 a = verts[S.vert_off + (k - D.n_vert)];
          for (int i = 0; i < 3; ++i) p[i] = ((B[3 * i] * a.x + B[3 * i + 1] * a.y) + B[3 * i + 2] * a.z) + B[9 + i];
          const float u[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
          for (int i = 0; i < 3; ++i) ploc[i] = (R[i] * u[0] + R[3 + i] * u[1]) + R[6 + i] * u[2];
          pl = s_dp; npl = D.n_plane; sgn = -1.f; Rn = s_R;
        }
        float best = -INFINITY;
        int bf = -1;
        bool in = true;
        for (int f = 0; f < npl; ++f) {
          const float4 e = pl[f];
          const float s = ((e.x * ploc[0] + e.y * ploc[1]) + e.z * ploc[2]) - e.w;
          if (s >= m) { in = false; break; }
          if (s > best) { best = s; bf = f; }
        }
        if (!in || bf < 0) continue;
        const float4 e = pl[bf];
        float nw[3];
        for (int i = 0; i < 3; ++i) {
          const float t = (Rn[3 * i] * e.x + Rn[3 * i + 1] * e.y) + Rn[3 * i + 2] * e.z;
          nw[i] = sgn < 0.f ? -t : t;
        }
        fl[h] = true;
        cp[h] = make_float4(p[0], p[1], p[2], best - m);
        cn[h] = make_float4(nw[0], nw[1], nw[2], 0.f);
      }
      const unsigned long long b0 = __ballot(fl[0]), b1 = __ballot(fl[1]);
      if (lane == 0) { s_wc[wv] = __popcll(b0); s_wc[4 + wv] = __popcll(b1); }
      __syncthreads();
      int cnt = 0, base0 = 0, base1 = 0;
      for (int k = 0; k < 8; ++k) {
        if (k == wv) base0 = cnt;
        if (k == 4 + wv) base1 = cnt;
        cnt += s_wc[k];
      }
      if (fl[0]) { const int at = base0 + wave::rank_in(b0, lane); s_cp[at] = cp[0]; s_cn[at] = cn[0]; }
      if (fl[1]) { const int at = base1 + wave::rank_in(b1, lane); s_cp[at] = cp[1]; s_cn[at] = cn[1]; }
      __syncthreads();
      if constexpr (EDGES) {
        // 3e: edge-edge candidates, appended after the vertex candidates
        __shared__ unsigned short s_ae[2][MAXE];   // active edges of D ([0]) and of S ([1]), ascending edge index
        const PhysEdgeSlice Der = s_er[0], Ser = s_er[1 + b];
        int n_act[2];
        for (int side = 0; side < 2; ++side) {
          // an edge is active unless one plane of the other body holds both its end points at s_f >= m
          const int ne = side == 0 ? Der.n_edge : Ser.n_edge;
          const int eoff = side == 0 ? Der.edge_off : Ser.edge_off;
          const float4* pl = side == 0 ? s_sp : s_dp;
          const int npl = side == 0 ? S.n_plane : D.n_plane;
          int na = 0;
          for (int e0 = 0; e0 < ne; e0 += PT) {
            const int e = e0 + tid;
            bool act = false;
            if (e < ne) {
              const int4 row = edges[eoff + e];
              float la[3], lb[3];
              if (side == 0) {
                const float4 a = s_dw[row.x], c = s_dw[row.y];
                const float ua[3] = {a.x - B[9], a.y - B[10], a.z - B[11]}, ub[3] = {c.x - B[9], c.y - B[10], c.z - B[11]};
                for (int i = 0; i < 3; ++i) {
                  la[i] = (B[i] * ua[0] + B[3 + i] * ua[1]) + B[6 + i] * ua[2];
                  lb[i] = (B[i] * ub[0] + B[3 + i] * ub[1]) + B[6 + i] * ub[2];
                }
              } else {
                const float4 a = verts[S.vert_off + row.x], c = verts[S.vert_off + row.y];
                float ua[3], ub[3];
                for (int i = 0; i < 3; ++i) {
                  ua[i] = (((B[3 * i] * a.x + B[3 * i + 1] * a.y) + B[3 * i + 2] * a.z) + B[9 + i]) - x[i];
                  ub[i] = (((B[3 * i] * c.x + B[3 * i + 1] * c.y) + B[3 * i + 2] * c.z) + B[9 + i]) - x[i];
                }
                for (int i = 0; i < 3; ++i) {
                  la[i] = (R[i] * ua[0] + R[3 + i] * ua[1]) + R[6 + i] * ua[2];
                  lb[i] = (R[i] * ub[0] + R[3 + i] * ub[1]) + R[6 + i] * ub[2];
                }
              }
              act = true;
              for (int f = 0; f < npl; ++f) {
                const float4 q = pl[f];
                const float sa = ((q.x * la[0] + q.y * la[1]) + q.z * la[2]) - q.w;
                const float sb = ((q.x * lb[0] + q.y * lb[1]) + q.z * lb[2]) - q.w;
                if (sa >= m && sb >= m) { act = false; break; }
              }
            }
            const unsigned long long ba = __ballot(act);
            if (lane == 0) s_wc[wv] = __popcll(ba);
            __syncthreads();
            int at = na;
            for (int k = 0; k < 4; ++k) {
              if (k < wv) at += s_wc[k];
              na += s_wc[k];
            }
            if (act) s_ae[side][at + wave::rank_in(ba, lane)] = (unsigned short)e;
            __syncthreads();
          }
          n_act[side] = na;
        }
        // pairs in ascending (active D edge, active S edge) order, one per thread, a workgroup's worth at a time
        const int npair = n_act[0] * n_act[1];
        const float reach2 = reach * reach;
        for (int p0 = 0; p0 < npair && cnt < 2 * PT; p0 += PT) {
          const int pi = p0 + tid;
          bool ok = false;
          float4 ecp = make_float4(0.f, 0.f, 0.f, 0.f), ecn = ecp;
          if (pi < npair) {
            const int ia = pi / n_act[1];
            const int4 ed = edges[Der.edge_off + s_ae[0][ia]], es = edges[Ser.edge_off + s_ae[1][pi - ia * n_act[1]]];
            const float4 a0 = s_dw[ed.x], a1 = s_dw[ed.y];
            const float4 v0 = verts[S.vert_off + es.x], v1 = verts[S.vert_off + es.y];
            float b0[3], b1v[3];
            for (int i = 0; i < 3; ++i) {
              b0[i] = ((B[3 * i] * v0.x + B[3 * i + 1] * v0.y) + B[3 * i + 2] * v0.z) + B[9 + i];
              b1v[i] = ((B[3 * i] * v1.x + B[3 * i + 1] * v1.y) + B[3 * i + 2] * v1.z) + B[9 + i];
            }
            const float d1[3] = {a1.x - a0.x, a1.y - a0.y, a1.z - a0.z};
            const float d2[3] = {b1v[0] - b0[0], b1v[1] - b0[1], b1v[2] - b0[2]};
            const float r[3] = {a0.x - b0[0], a0.y - b0[1], a0.z - b0[2]};
            const float a = dot3(d1, d1), e = dot3(d2, d2), bq = dot3(d1, d2), c = dot3(d1, r), f = dot3(d2, r);
            const float ae = a * e;
            const float den = ae - bq * bq;
            if (den > 1e-6f * ae) {
              const float s = fdv(bq * f - c * e, den), t = fdv(a * f - bq * c, den);
              if (s > 0.f && s < 1.f && t > 0.f && t < 1.f) {
                const float cD[3] = {a0.x + s * d1[0], a0.y + s * d1[1], a0.z + s * d1[2]};
                const float cS[3] = {b0[0] + t * d2[0], b0[1] + t * d2[1], b0[2] + t * d2[2]};
                const float g[3] = {cD[0] - cS[0], cD[1] - cS[1], cD[2] - cS[2]};
                if (!(norm2_3(g[0], g[1], g[2]) > reach2)) {
                  // c_D inside S grown by m, c_S inside D grown by m
                  const float uS[3] = {cD[0] - B[9], cD[1] - B[10], cD[2] - B[11]};
                  const float uD[3] = {cS[0] - x[0], cS[1] - x[1], cS[2] - x[2]};
                  float lS[3], lD[3];
                  for (int i = 0; i < 3; ++i) {
                    lS[i] = (B[i] * uS[0] + B[3 + i] * uS[1]) + B[6 + i] * uS[2];
                    lD[i] = (R[i] * uD[0] + R[3 + i] * uD[1]) + R[6 + i] * uD[2];
                  }
                  bool in = true;
                  for (int k = 0; k < S.n_plane && in; ++k) {
                    const float4 q = s_sp[k];
                    in = ((q.x * lS[0] + q.y * lS[1]) + q.z * lS[2]) - q.w < m;
                  }
                  for (int k = 0; k < D.n_plane && in; ++k) {
                    const float4 q = s_dp[k];
                    in = ((q.x * lD[0] + q.y * lD[1]) + q.z * lD[2]) - q.w < m;
                  }
                  if (in) {
                    float cr[3], n[3];
                    cross3(d1, d2, cr);
                    const float L = fsq(norm2_3(cr[0], cr[1], cr[2]));
                    for (int i = 0; i < 3; ++i) n[i] = fdv(cr[i], L);
                    const float4 s0 = s_sp[es.z], s1 = s_sp[es.w], q0 = s_dp[ed.z], q1 = s_dp[ed.w];
                    const float qS[3] = {s0.x + s1.x, s0.y + s1.y, s0.z + s1.z}, qD[3] = {q0.x + q1.x, q0.y + q1.y, q0.z + q1.z};
                    float oS[3], oD[3];
                    for (int i = 0; i < 3; ++i) {
                      oS[i] = (B[3 * i] * qS[0] + B[3 * i + 1] * qS[1]) + B[3 * i + 2] * qS[2];
                      oD[i] = (R[3 * i] * qD[0] + R[3 * i + 1] * qD[1]) + R[3 * i + 2] * qD[2];
                    }
                    float dS = dot3(n, oS), dD = dot3(n, oD);
                    if (dS < 0.f) {
                      for (int i = 0; i < 3; ++i) n[i] = -n[i];
                      dS = -dS; dD = -dD;
                    }
                    if (dS > 0.f && dD < 0.f) {
                      ok = true;
                      ecp = make_float4(cD[0], cD[1], cD[2], dot3(n, g) - m);
                      ecn = make_float4(n[0], n[1], n[2], 0.f);
                    }
                  }
                }
              }
            }
          }
          const unsigned long long bo = __ballot(ok);
          if (lane == 0) s_wc[wv] = __popcll(bo);
          __syncthreads();
          int at = cnt;
          for (int k = 0; k < 4; ++k) {
            if (k < wv) at += s_wc[k];
            cnt += s_wc[k];
          }
          at += wave::rank_in(bo, lane);
          if (ok && at < 2 * PT) { s_cp[at] = ecp; s_cn[at] = ecn; }   // past the capacity: dropped, in pair order
          if (cnt > 2 * PT) cnt = 2 * PT;
          __syncthreads();
        }
      }
      if (cnt > 4) {
        for (int round = 0; round < 4; ++round) {
          float bv = -INFINITY;
          int bi = INT_MAX;
          for (int h = 0; h < 2; ++h) {
            const int k = h * PT + tid;
            if (k >= cnt) continue;
            bool taken = false;
            for (int r = 0; r < round; ++r) taken |= (s_pick[r] == k);
            if (taken) continue;
            const float4 c = s_cp[k];
            float val;
            if (round == 0) {
              val = -c.w;
            } else {
              const float4 p1 = s_cp[s_pick[0]];
              const float a[3] = {c.x - p1.x, c.y - p1.y, c.z - p1.z};
              if (round == 1) {
                val = norm2_3(a[0], a[1], a[2]);
              } else {
                const float4 p2 = s_cp[s_pick[1]];
                const float bb[3] = {c.x - p2.x, c.y - p2.y, c.z - p2.z};
                float o[3];
                cross3(a, bb, o);
                val = norm2_3(o[0], o[1], o[2]);
                if (round == 3) {
                  const float4 p3 = s_cp[s_pick[2]];
                  const float cc[3] = {c.x - p3.x, c.y - p3.y, c.z - p3.z};
                  float o2[3], o3[3];
                  cross3(bb, cc, o2);
                  cross3(cc, a, o3);
                  val = (val + norm2_3(o2[0], o2[1], o2[2])) + norm2_3(o3[0], o3[1], o3[2]);
                }
              }
            }
            if (better(val, k, bv, bi)) { bv = val; bi = k; }
          }
          for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
          }
          if (lane == 0) { s_rv[wv] = bv; s_ri[wv] = bi; }
          __syncthreads();
          if (tid == 0) {
            float fv = s_rv[0];
            int fi = s_ri[0];
            for (int k = 1; k < 4; ++k)
              if (better(s_rv[k], s_ri[k], fv, fi)) { fv = s_rv[k]; fi = s_ri[k]; }
            s_pick[round] = fi;
          }
          __syncthreads();
        }
      }
      if (tid == 0) {
        const int take = cnt > 4 ? 4 : cnt;
        for (int r = 0; r < take; ++r) {
          const int k = cnt > 4 ? s_pick[r] : r;
          s_ctp[s_nct] = s_cp[k];
          s_ctn[s_nct] = s_cn[k];
          ++s_nct;
        }
      }
      __syncthreads();
    }

    // 5-6: sequential impulses and integration, one lane
    if (tid == 0) {
      const int nc = s_nct;
      float v[3] = {s_v[0], s_v[1], s_v[2]}, w[3] = {s_w[0], s_w[1], s_w[2]};
      float Iw[9];
      for (int k = 0; k < 9; ++k) Iw[k] = s_Iw[k];
      for (int c = 0; c < nc; ++c) {
        const float4 p = s_ctp[c], n4 = s_ctn[c];
        const float r[3] = {p.x - x[0], p.y - x[1], p.z - x[2]};
        const float n[3] = {n4.x, n4.y, n4.z};
        float tg = fdv((-p.w) * P.erp, P.dt);
        if (tg < 0.f) tg = 0.f;
        row_build(s_rows[c], r, n, Iw, tg);
        float t1[3], t2[3];
        plane_space(n, t1, t2);
        row_build(s_rows[MAXC + 2 * c], r, t1, Iw, 0.f);
        row_build(s_rows[MAXC + 2 * c + 1], r, t2, Iw, 0.f);
      }
      for (int it = 0; it < P.iterations; ++it) {
        for (int c = 0; c < nc; ++c) row_solve(s_rows[c], 0.f, INFINITY, v, w);
        for (int c = 0; c < nc; ++c) {
          const float lim = P.mu * s_rows[c].lambda;
          row_solve(s_rows[MAXC + 2 * c], -lim, lim, v, w);
          row_solve(s_rows[MAXC + 2 * c + 1], -lim, lim, v, w);
        }
      }
      float q[4] = {s_q[0], s_q[1], s_q[2], s_q[3]};
      for (int i = 0; i < 3; ++i) x[i] = x[i] + P.dt * v[i];
      const float o[4] = {(w[0] * q[3] + w[1] * q[2]) - w[2] * q[1], (w[1] * q[3] + w[2] * q[0]) - w[0] * q[2],
                          (w[2] * q[3] + w[0] * q[1]) - w[1] * q[0], -((w[0] * q[0] + w[1] * q[1]) + w[2] * q[2])};
      for (int i = 0; i < 4; ++i) q[i] = q[i] + P.half_dt * o[i];
      const float qn = fsq(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
      for (int i = 0; i < 4; ++i) s_q[i] = fdv(q[i], qn);
      for (int i = 0; i < 3; ++i) { s_x[i] = x[i]; s_v[i] = v[i]; s_w[i] = w[i]; }
      if (tr_state) {
        float* ts = tr_state + (size_t)step * TRACE_STATE;
        for (int i = 0; i < 3; ++i) ts[i] = s_x[i];
        for (int i = 0; i < 4; ++i) ts[3 + i] = s_q[i];
        for (int i = 0; i < 3; ++i) { ts[7 + i] = v[i]; ts[10 + i] = w[i]; }
        float* tc = tr_contacts + (size_t)step * MAXC * TRACE_CONTACT;
        for (int c = 0; c < nc; ++c) {
          const float4 p = s_ctp[c], n4 = s_ctn[c];
          const float e[8] = {p.x, p.y, p.z, n4.x, n4.y, n4.z, p.w, s_rows[c].lambda};
          for (int k = 0; k < 8; ++k) tc[c * TRACE_CONTACT + k] = e[k];
        }
        tr_n[step] = nc;
      }
    }
    __syncthreads();
  }

  if (tid == 0) {
    float R[9], W[16], O[16];
    R_from_q(s_q, R);
    for (int i = 0; i < 3; ++i) {
      for (int c = 0; c < 3; ++c) W[c * 4 + i] = R[3 * i + c];
      W[12 + i] = s_x[i];
      W[i * 4 + 3] = 0.f;
    }
    W[15] = 1.f;
    if (P.has_cam) mat4_mul(P.cam_inv, W, O);
    else
      for (int e = 0; e < 16; ++e) O[e] = W[e];
    for (int e = 0; e < 16; ++e) T_out[(size_t)st * 16 + e] = O[e];
    if (info) {
      pgp_physics_info inf;
      const int nc = s_nct;
      float md = 0.f;
      for (int c = 0; c < nc; ++c) md = fminf(md, s_ctp[c].w);
      inf.n_contacts = nc;
      inf.min_depth = md;
      inf.lin_speed = fsq(norm2_3(s_v[0], s_v[1], s_v[2]));
      inf.ang_speed = fsq(norm2_3(s_w[0], s_w[1], s_w[2]));
      info[st] = inf;
    }
  }
}

// ---- step 3p: polyhedral contacts (pgp_physics_set_polyhedral_contacts) -------------------------------------------------
// A sibling of settle_kernel, not a third instantiation: the two instantiations above compile from the source they had.
// Steps 1, 2, 4, 5 and 6 below are that kernel's text; step 3p stands where its steps 3 and 3e stand.
constexpr int MAXPOLY = 2 * PT;   // polygon and candidate capacity of a pair
constexpr int EROW = 12;          // floats of a staged edge: world end points (3 + 3), the two world normals (3 + 3)

// block arg-max with lowest-index ties over the (v, i) of all 256 threads; every thread leaves with the winner.
// sv / si: 4 LDS entries each, free to be overwritten once every thread has arrived
__device__ __forceinline__ void block_argmax(float& v, int& i, float* sv, int* si) {
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (better(ov, oi, v, i)) { v = ov; i = oi; }
  }
  __syncthreads();
  if (wave::lane() == 0) si[wave::wave_id()] = i;
  wave::block4_publish(sv, wave::lane() == 0, v);
  v = sv[0]; i = si[0];
  for (int k = 1; k < 4; ++k)
    if (better(sv[k], si[k], v, i)) { v = sv[k]; i = si[k]; }
}

// the face query of one body: sep(f) = the least s_f over the other body's vertices loc[0 .. nv) (in this body's frame),
// one plane per thread; leaves the first maximal sep in bv, its plane in bi and the vertex that attained it (the first
// minimum) in vtx
__device__ __forceinline__ void face_query(const float4* pl, int npl, const float4* loc, int nv, int* sepv, float* sv, int* si,
                                           float& bv, int& bi, int& vtx) {
  bv = -INFINITY;
  bi = INT_MAX;
  for (int f = threadIdx.x; f < npl; f += PT) {
    const float4 e = pl[f];
    float mn = INFINITY;
    int mi = 0;
    for (int i = 0; i < nv; ++i) {
      const float4 p = loc[i];
      const float s = ((e.x * p.x + e.y * p.y) + e.z * p.z) - e.w;
      if (s < mn) { mn = s; mi = i; }
    }
    sepv[f] = mi;
    if (mn > bv) { bv = mn; bi = f; }
  }
  block_argmax(bv, bi, sv, si);
  vtx = bi < npl ? sepv[bi] : 0;
}

// the edge axis of one pair (a of D, b of S; ea / eb their staged rows): false when the arcs of their planes' normals do
// not cross on the Gauss map, when the edges are parallel or when n does not leave S and enter D
__device__ __forceinline__ bool edge_axis(const float* ea, const float* eb, const int4* rowD, const int4* rowS, const float4* dp,
                                          const float4* sp, const float* R, const float* B, float* n, float& sep, float* d1,
                                          float* d2, float* r, float& den) {
  const float *A = ea + 6, *Bn = ea + 9, *C = eb + 6, *E = eb + 9;
  float bxa[3], exc[3];
  cross3(Bn, A, bxa);
  cross3(E, C, exc);
  const float cba = dot3(C, bxa), dba = dot3(E, bxa), adc = dot3(A, exc), bdc = dot3(Bn, exc);
  if (!(cba * dba < 0.f && adc * bdc < 0.f && cba * bdc > 0.f)) return false;
  for (int i = 0; i < 3; ++i) { d1[i] = ea[3 + i] - ea[i]; d2[i] = eb[3 + i] - eb[i]; r[i] = ea[i] - eb[i]; }
  const float a = dot3(d1, d1), e = dot3(d2, d2), bq = dot3(d1, d2);
  const float ae = a * e;
  den = ae - bq * bq;
  if (!(den > 1e-6f * ae)) return false;
  float cr[3];
  cross3(d1, d2, cr);
  const float L = fsq(norm2_3(cr[0], cr[1], cr[2]));
  for (int i = 0; i < 3; ++i) n[i] = fdv(cr[i], L);
  const int4 ed = *rowD, es = *rowS;
  const float4 s0 = sp[es.z], s1 = sp[es.w], q0 = dp[ed.z], q1 = dp[ed.w];
  const float qS[3] = {s0.x + s1.x, s0.y + s1.y, s0.z + s1.z}, qD[3] = {q0.x + q1.x, q0.y + q1.y, q0.z + q1.z};
  float oS[3], oD[3];
  for (int i = 0; i < 3; ++i) {
    oS[i] = (B[3 * i] * qS[0] + B[3 * i + 1] * qS[1]) + B[3 * i + 2] * qS[2];
    oD[i] = (R[3 * i] * qD[0] + R[3 * i + 1] * qD[1]) + R[3 * i + 2] * qD[2];
  }
  float dS = dot3(n, oS), dD = dot3(n, oD);
  if (dS < 0.f) {
    for (int i = 0; i < 3; ++i) n[i] = -n[i];
    dS = -dS; dD = -dD;
  }
  if (!(dS > 0.f && dD < 0.f)) return false;
  sep = dot3(n, r);
  return true;
}

__global__ void __launch_bounds__(PT) settle_poly_kernel(PhysParams P, const PhysShape* __restrict__ shapes,
                                                         const float4* __restrict__ verts, const float4* __restrict__ planes,
                                                         const int* __restrict__ dyn_shape, const float* T,
                                                         const int* __restrict__ static_off, const int* __restrict__ static_shape,
                                                         const float* __restrict__ static_T, float* T_out,
                                                         pgp_physics_info* __restrict__ info, float* __restrict__ tr_state,
                                                         float* __restrict__ tr_contacts, int* __restrict__ tr_n,
                                                         const PhysEdgeSlice* __restrict__ eslice, const int4* __restrict__ edges,
                                                         const PhysFaceSlice* __restrict__ fslice, const int* __restrict__ foff,
                                                         const int* __restrict__ fidx, float face_bias) {
  __shared__ float4 s_dv[MAXV];        // D's hull, body frame
  __shared__ float4 s_dw[MAXV];        // D's hull, world frame of the step
  __shared__ float4 s_dp[MAXP];        // D's planes, body frame
  __shared__ float4 s_sp[MAXP];        // the planes of the pair's static body S, body frame
  __shared__ float4 s_pa[MAXPOLY];     // the polygon under the clipping; the candidates: point (xyz), depth (w)
  __shared__ float4 s_pb[MAXPOLY];     // its other half: each pass reads one and writes the other
  __shared__ float4 s_loc[MAXV];       // the face queries: the other body's vertices in the frame of the planes
  __shared__ int s_sepv[MAXP];         // the face queries: per plane, the vertex that attained sep
  __shared__ float s_ed[MAXE * EROW];  // D's edges of the step: a0, a1, A, B (world)
  __shared__ float s_es[MAXE * EROW];  // S's edges of the pair: b0, b1, C, E (world, the normals negated)
  __shared__ float s_body[MAXB][12];   // R (row-major) | t of the table and the statics, world frame
  __shared__ PhysShape s_sh[MAXB + 1]; // [0] = D, [1 + j] = body j
  __shared__ PhysEdgeSlice s_er[MAXB + 1];
  __shared__ PhysFaceSlice s_fs[MAXB + 1];
  __shared__ float4 s_ctp[MAXC], s_ctn[MAXC];
  __shared__ Row s_rows[3 * MAXC];
  __shared__ float s_x[3], s_q[4], s_v[3], s_w[3], s_R[9], s_Iw[9], s_Tin[16], s_pn[3];
  __shared__ int s_ok, s_nb, s_nct, s_pick[4], s_ri[4];
  __shared__ uint32_t s_sc[4];
  __shared__ float s_rv[4];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int st = blockIdx.x;
  if (st >= P.n_states) return;

  if (tid == 0) {
    int ok = 1;
    const int dyn = dyn_shape[st];
    const int o0 = static_off[st], o1 = static_off[st + 1];
    if (dyn < 0 || dyn >= P.n_shapes || o0 < 0 || o1 < o0 || o1 - o0 > PGP_PHYSICS_MAX_STATICS) ok = 0;
    if (ok)
      for (int k = o0; k < o1; ++k)
        if (static_shape[k] < 0 || static_shape[k] >= P.n_shapes) ok = 0;
    for (int k = 0; k < 16; ++k) {
      s_Tin[k] = T[(size_t)st * 16 + k];
      if (!isfinite(s_Tin[k])) ok = 0;
    }
    if (ok) {
      s_sh[0] = shapes[dyn];
      s_sh[1] = shapes[0];
      s_er[0] = eslice[dyn];
      s_er[1] = eslice[0];
      s_fs[0] = fslice[dyn];
      s_fs[1] = fslice[0];
      for (int i = 0; i < 3; ++i) {
        for (int c = 0; c < 3; ++c) s_body[0][3 * i + c] = P.table[4 * i + c];
        s_body[0][9 + i] = P.table[4 * i + 3];
      }
      for (int k = o0; k < o1; ++k) {
        const int b = 1 + (k - o0);
        s_sh[1 + b] = shapes[static_shape[k]];
        s_er[1 + b] = eslice[static_shape[k]];
        s_fs[1 + b] = fslice[static_shape[k]];
        float Ts[16], W[16];
        for (int e = 0; e < 16; ++e) Ts[e] = static_T[(size_t)k * 16 + e];
        if (P.has_cam) mat4_mul(P.cam, Ts, W);
        else
          for (int e = 0; e < 16; ++e) W[e] = Ts[e];
        for (int i = 0; i < 3; ++i) {
          for (int c = 0; c < 3; ++c) s_body[b][3 * i + c] = W[c * 4 + i];
          s_body[b][9 + i] = W[12 + i];
        }
      }
      s_nb = 1 + (o1 - o0);
      float W[16];
      if (P.has_cam) mat4_mul(P.cam, s_Tin, W);
      else
        for (int e = 0; e < 16; ++e) W[e] = s_Tin[e];
      float R[9];
      for (int i = 0; i < 3; ++i)
        for (int c = 0; c < 3; ++c) R[3 * i + c] = W[c * 4 + i];
      quat_from_R(R, s_q);
      for (int i = 0; i < 3; ++i) { s_x[i] = W[12 + i]; s_v[i] = 0.f; s_w[i] = 0.f; }
    }
    s_ok = ok;
  }
  __syncthreads();
  if (!s_ok || P.steps == 0) {
    if (tid < 16) T_out[(size_t)st * 16 + tid] = s_ok ? s_Tin[tid] : __int_as_float(0x7fc00000);
    if (tid == 0 && info) {
      pgp_physics_info inf;
      inf.n_contacts = s_ok ? 0 : -1;
      inf.min_depth = 0.f; inf.lin_speed = 0.f; inf.ang_speed = 0.f;
      info[st] = inf;
    }
    return;
  }
  const PhysShape D = s_sh[0];
  const PhysEdgeSlice Der = s_er[0];
  const PhysFaceSlice Dfs = s_fs[0];
  const int nD = min(Der.n_edge, MAXE);
  for (int i = tid; i < D.n_vert; i += PT) s_dv[i] = verts[D.vert_off + i];
  for (int f = tid; f < D.n_plane; f += PT) s_dp[f] = planes[D.plane_off + f];
  const float inv_i[3] = {fdv(1.f, D.inertia[0]), fdv(1.f, D.inertia[1]), fdv(1.f, D.inertia[2])};
  const int nb = s_nb;

  for (int step = 0; step < P.steps; ++step) {
    // 1-2: velocities, damping, clamp; R, Iw
    if (tid == 0) {
      float* v = s_v; float* w = s_w;
      for (int i = 0; i < 3; ++i) v[i] = (v[i] + P.dt * P.g[i]) * P.lin_c;
      for (int i = 0; i < 3; ++i) w[i] = w[i] * P.ang_c;
      const float L = fsq(norm2_3(w[0], w[1], w[2]));
      if (L * P.dt > HALF_PI_F) {
        const float sc = fdv(P.w_max, L);
        for (int i = 0; i < 3; ++i) w[i] = w[i] * sc;
      }
      R_from_q(s_q, s_R);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          s_Iw[3 * i + j] = ((s_R[3 * i] * inv_i[0]) * s_R[3 * j] + (s_R[3 * i + 1] * inv_i[1]) * s_R[3 * j + 1]) +
                            (s_R[3 * i + 2] * inv_i[2]) * s_R[3 * j + 2];
      s_nct = 0;
    }
    __syncthreads();
    float R[9], x[3];
    for (int k = 0; k < 9; ++k) R[k] = s_R[k];
    for (int k = 0; k < 3; ++k) x[k] = s_x[k];
    for (int i = tid; i < D.n_vert; i += PT) {
      const float4 a = s_dv[i];
      s_dw[i] = make_float4(((R[0] * a.x + R[1] * a.y) + R[2] * a.z) + x[0], ((R[3] * a.x + R[4] * a.y) + R[5] * a.z) + x[1],
                            ((R[6] * a.x + R[7] * a.y) + R[8] * a.z) + x[2], 0.f);
    }
    __syncthreads();
    // D's edges of the step: world end points and the world normals A, B of their two planes
    for (int e = tid; e < nD; e += PT) {
      const int4 row = edges[Der.edge_off + e];
      const float4 a0 = s_dw[row.x], a1 = s_dw[row.y], n0 = s_dp[row.z], n1 = s_dp[row.w];
      float* o = s_ed + e * EROW;
      o[0] = a0.x; o[1] = a0.y; o[2] = a0.z; o[3] = a1.x; o[4] = a1.y; o[5] = a1.z;
      for (int i = 0; i < 3; ++i) {
        o[6 + i] = (R[3 * i] * n0.x + R[3 * i + 1] * n0.y) + R[3 * i + 2] * n0.z;
        o[9 + i] = (R[3 * i] * n1.x + R[3 * i + 1] * n1.y) + R[3 * i + 2] * n1.z;
      }
    }

    // 3p-4: contacts pair by pair
    for (int b = 0; b < nb; ++b) {
      const PhysShape S = s_sh[1 + b];
      const float* B = s_body[b];
      const float m = D.margin + S.margin;
      {
        const float dx = B[9] - x[0], dy = B[10] - x[1], dz = B[11] - x[2];
        const float rr = (D.radius + S.radius) + m;
        if (norm2_3(dx, dy, dz) > rr * rr) continue;   // uniform over the block
      }
      const PhysEdgeSlice Ser = s_er[1 + b];
      const PhysFaceSlice Sfs = s_fs[1 + b];
      const int nS = min(Ser.n_edge, MAXE);
      // S's world vertex i
      const auto s_world = [&](int i, float* p) {
        const float4 a = verts[S.vert_off + i];
        for (int c = 0; c < 3; ++c) p[c] = ((B[3 * c] * a.x + B[3 * c + 1] * a.y) + B[3 * c + 2] * a.z) + B[9 + c];
      };
      __syncthreads();   // the pair before is done with s_sp, s_loc, s_es and the polygons; s_ed is written
      for (int f = tid; f < S.n_plane; f += PT) s_sp[f] = planes[S.plane_off + f];
      // face query of S's planes over D's vertices
      for (int i = tid; i < D.n_vert; i += PT) {
        const float4 a = s_dw[i];
        const float u[3] = {a.x - B[9], a.y - B[10], a.z - B[11]};
        s_loc[i] = make_float4((B[0] * u[0] + B[3] * u[1]) + B[6] * u[2], (B[1] * u[0] + B[4] * u[1]) + B[7] * u[2],
                               (B[2] * u[0] + B[5] * u[1]) + B[8] * u[2], 0.f);
      }
      __syncthreads();
      float bvS, bvD;
      int biS, biD, vS, vD;
      face_query(s_sp, S.n_plane, s_loc, D.n_vert, s_sepv, s_rv, s_ri, bvS, biS, vS);
      __syncthreads();
      // face query of D's planes over S's vertices
      for (int i = tid; i < S.n_vert; i += PT) {
        float p[3];
        s_world(i, p);
        const float u[3] = {p[0] - x[0], p[1] - x[1], p[2] - x[2]};
        s_loc[i] = make_float4((R[0] * u[0] + R[3] * u[1]) + R[6] * u[2], (R[1] * u[0] + R[4] * u[1]) + R[7] * u[2],
                               (R[2] * u[0] + R[5] * u[1]) + R[8] * u[2], 0.f);
      }
      __syncthreads();
      face_query(s_dp, D.n_plane, s_loc, S.n_vert, s_sepv, s_rv, s_ri, bvD, biD, vD);
      if (bvS >= m || bvD >= m || biS >= S.n_plane || biD >= D.n_plane) continue;   // a separating face; uniform

      // edge query: S's edges of the pair, then one pair per thread and pass
      for (int e = tid; e < nS; e += PT) {
        const int4 row = edges[Ser.edge_off + e];
        const float4 n0 = s_sp[row.z], n1 = s_sp[row.w];
        float* o = s_es + e * EROW;
        s_world(row.x, o);
        s_world(row.y, o + 3);
        for (int i = 0; i < 3; ++i) {
          o[6 + i] = -((B[3 * i] * n0.x + B[3 * i + 1] * n0.y) + B[3 * i + 2] * n0.z);
          o[9 + i] = -((B[3 * i] * n1.x + B[3 * i + 1] * n1.y) + B[3 * i + 2] * n1.z);
        }
      }
      __syncthreads();
      const int npair = nD * nS;
      float bvE = -INFINITY;
      int biE = INT_MAX;
      for (int pi = tid; pi < npair; pi += PT) {
        const int ia = pi / nS, ib = pi - ia * nS;
        float n[3], d1[3], d2[3], r[3], sep, den;
        if (edge_axis(s_ed + ia * EROW, s_es + ib * EROW, edges + Der.edge_off + ia, edges + Ser.edge_off + ib, s_dp, s_sp, R, B,
                      n, sep, d1, d2, r, den) &&
            sep > bvE) {
          bvE = sep;
          biE = pi;
        }
      }
      block_argmax(bvE, biE, s_rv, s_ri);
      const bool has_edge = biE != INT_MAX;
      if (has_edge && bvE >= m) continue;   // a separating edge axis; uniform

      int cnt = 0;
      const float4* cand = s_pa;
      if (has_edge && bvE > fmaxf(bvS, bvD) + face_bias) {
        // edge contact: the closest point of D's edge, its parameter clamped to the segment
        if (tid == 0) {
          const int ia = biE / nS, ib = biE - ia * nS;
          float n[3], d1[3], d2[3], r[3], sep, den;
          edge_axis(s_ed + ia * EROW, s_es + ib * EROW, edges + Der.edge_off + ia, edges + Ser.edge_off + ib, s_dp, s_sp, R, B, n,
                    sep, d1, d2, r, den);
          const float e = dot3(d2, d2), bq = dot3(d1, d2), c = dot3(d1, r), f = dot3(d2, r);
          float s = fdv(bq * f - c * e, den);
          if (s < 0.f) s = 0.f;
          if (s > 1.f) s = 1.f;
          const float* a0 = s_ed + ia * EROW;
          s_pa[0] = make_float4(a0[0] + s * d1[0], a0[1] + s * d1[1], a0[2] + s * d1[2], bvE - m);
          for (int i = 0; i < 3; ++i) s_pn[i] = n[i];
        }
        cnt = 1;
      } else {
        // face contact: the reference plane f* of body S (best_S >= best_D) or D, the incident face of the other body
        const bool refS = bvS >= bvD;
        const int fr = refS ? biS : biD;
        const float4 e = refS ? s_sp[fr] : s_dp[fr];
        const float* Rr = refS ? B : s_R;
        const float* Ri = refS ? s_R : B;
        const float tr[3] = {refS ? B[9] : x[0], refS ? B[10] : x[1], refS ? B[11] : x[2]};
        float N[3];
        for (int i = 0; i < 3; ++i) N[i] = (Rr[3 * i] * e.x + Rr[3 * i + 1] * e.y) + Rr[3 * i + 2] * e.z;
        const float4* pli = refS ? s_dp : s_sp;
        const int npi = refS ? D.n_plane : S.n_plane;
        float bvI = -INFINITY;
        int g = INT_MAX;
        for (int f = tid; f < npi; f += PT) {
          const float4 q = pli[f];
          float w[3];
          for (int i = 0; i < 3; ++i) w[i] = (Ri[3 * i] * q.x + Ri[3 * i + 1] * q.y) + Ri[3 * i + 2] * q.z;
          const float val = -dot3(N, w);
          if (val > bvI) { bvI = val; g = f; }
        }
        block_argmax(bvI, g, s_rv, s_ri);
        if (g >= npi) continue;   // every N . n_g is NaN: no contact; uniform
        // a world vertex of the incident (inc) or the reference body
        const auto world_of = [&](bool of_S, int i, float* p) {
          if (of_S) {
            s_world(i, p);
          } else {
            const float4 a = s_dw[i];
            p[0] = a.x; p[1] = a.y; p[2] = a.z;
          }
        };
        const PhysFaceSlice ifs = refS ? Dfs : Sfs, rfs = refS ? Sfs : Dfs;
        const int i0 = foff[ifs.off_off + g], r0 = foff[rfs.off_off + fr];
        int n = min(foff[ifs.off_off + g + 1] - i0, MAXV);
        const int nr = min(foff[rfs.off_off + fr + 1] - r0, MAXV);
        const int nvi = refS ? D.n_vert : S.n_vert, nvr = refS ? S.n_vert : D.n_vert;
        for (int i = tid; i < n; i += PT) {
          float p[3];
          world_of(!refS, min(fidx[ifs.idx_off + i0 + i], nvi - 1), p);
          s_pa[i] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        float4 *pa = s_pa, *pb = s_pb;
        for (int k = 0; k < nr && n > 0; ++k) {
          float u[3], w[3], kk[3];
          world_of(refS, min(fidx[rfs.idx_off + r0 + k], nvr - 1), u);
          world_of(refS, min(fidx[rfs.idx_off + r0 + (k + 1 == nr ? 0 : k + 1)], nvr - 1), w);
          const float wu[3] = {w[0] - u[0], w[1] - u[1], w[2] - u[2]};
          cross3(wu, N, kk);
          uint32_t total = 0;
          for (int j0 = 0; j0 < n; j0 += PT) {
            const int j = j0 + tid;
            uint32_t c = 0;
            float4 first = make_float4(0.f, 0.f, 0.f, 0.f), second = first;   // a when kept, then the crossing
            if (j < n) {
              const float4 a = pa[j], q = pa[j + 1 == n ? 0 : j + 1];
              const float da[3] = {a.x - u[0], a.y - u[1], a.z - u[2]}, dq[3] = {q.x - u[0], q.y - u[1], q.z - u[2]};
              const float sa = dot3(kk, da), sb = dot3(kk, dq);
              const bool ina = sa <= 0.f, inb = sb <= 0.f;
              if (ina) { first = a; c = 1; }
              if (ina != inb) {
                const float t = fdv(sa, sa - sb);
                second = make_float4(a.x + t * (q.x - a.x), a.y + t * (q.y - a.y), a.z + t * (q.z - a.z), 0.f);
                if (!ina) first = second;
                ++c;
              }
            }
            const uint32_t incl = wave::scan_incl(c, lane);
            wave::block4_publish(s_sc, lane == 63, incl);
            const uint32_t at = total + wave::block4_offset(s_sc, wv, 0u) + incl - c;
            // past the capacity: dropped, in output order
            if (c > 0 && at < (uint32_t)MAXPOLY) pb[at] = first;
            if (c > 1 && at + 1 < (uint32_t)MAXPOLY) pb[at + 1] = second;
            total += wave::block4_total(s_sc);
            __syncthreads();
          }
          n = (int)min(total, (uint32_t)MAXPOLY);
          float4* sw = pa; pa = pb; pb = sw;
        }
        if (n == 0) {
          // nothing left of the incident face: the incident body's vertex that attained sep
          if (tid == 0) {
            float p[3];
            world_of(!refS, refS ? vS : vD, p);
            pb[0] = make_float4(p[0], p[1], p[2], (refS ? bvS : bvD) - m);
          }
          cnt = 1;
        } else {
          // candidates: the clipped points below the margin over f*, in output order
          uint32_t total = 0;
          for (int j0 = 0; j0 < n; j0 += PT) {
            const int j = j0 + tid;
            bool fl = false;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < n) {
              a = pa[j];
              const float u[3] = {a.x - tr[0], a.y - tr[1], a.z - tr[2]};
              float loc[3];
              for (int i = 0; i < 3; ++i) loc[i] = (Rr[i] * u[0] + Rr[3 + i] * u[1]) + Rr[6 + i] * u[2];
              const float s = ((e.x * loc[0] + e.y * loc[1]) + e.z * loc[2]) - e.w;
              fl = s < m;
              a.w = s - m;
            }
            const unsigned long long bal = __ballot(fl);
            wave::block4_publish(s_sc, lane == 0, (uint32_t)__popcll(bal));
            if (fl) pb[wave::block4_rank(s_sc, bal, total)] = a;
            total += wave::block4_total(s_sc);
            __syncthreads();
          }
          cnt = (int)total;
        }
        cand = pb;
        if (tid == 0)
          for (int i = 0; i < 3; ++i) s_pn[i] = refS ? N[i] : -N[i];
      }
      __syncthreads();
      if (cnt > 4) {
        for (int round = 0; round < 4; ++round) {
          float bv = -INFINITY;
          int bi = INT_MAX;
          for (int h = 0; h < 2; ++h) {
            const int k = h * PT + tid;
            if (k >= cnt) continue;
            bool taken = false;
            for (int r = 0; r < round; ++r) taken |= (s_pick[r] == k);
            if (taken) continue;
            const float4 c = cand[k];
            float val;
            if (round == 0) {
              val = -c.w;
            } else {
              const float4 p1 = cand[s_pick[0]];
              const float a[3] = {c.x - p1.x, c.y - p1.y, c.z - p1.z};
              if (round == 1) {
                val = norm2_3(a[0], a[1], a[2]);
              } else {
                const float4 p2 = cand[s_pick[1]];
                const float bb[3] = {c.x - p2.x, c.y - p2.y, c.z - p2.z};
                float o[3];
                cross3(a, bb, o);
                val = norm2_3(o[0], o[1], o[2]);
                if (round == 3) {
                  const float4 p3 = cand[s_pick[2]];
                  const float cc[3] = {c.x - p3.x, c.y - p3.y, c.z - p3.z};
                  float o2[3], o3[3];
                  cross3(bb, cc, o2);
                  cross3(cc, a, o3);
                  val = (val + norm2_3(o2[0], o2[1], o2[2])) + norm2_3(o3[0], o3[1], o3[2]);
                }
              }
            }
            if (better(val, k, bv, bi)) { bv = val; bi = k; }
          }
          block_argmax(bv, bi, s_rv, s_ri);
          if (tid == 0) s_pick[round] = bi;
          __syncthreads();
        }
      }
      if (tid == 0) {
        const int take = cnt > 4 ? 4 : cnt;
        for (int r = 0; r < take; ++r) {
          const int k = cnt > 4 ? s_pick[r] : r;
          s_ctp[s_nct] = cand[k];
          s_ctn[s_nct] = make_float4(s_pn[0], s_pn[1], s_pn[2], 0.f);
          ++s_nct;
        }
      }
    }
    __syncthreads();

    // 5-6: sequential impulses and integration, one lane
    if (tid == 0) {
      const int nc = s_nct;
      float v[3] = {s_v[0], s_v[1], s_v[2]}, w[3] = {s_w[0], s_w[1], s_w[2]};
      float Iw[9];
      for (int k = 0; k < 9; ++k) Iw[k] = s_Iw[k];
      for (int c = 0; c < nc; ++c) {
        const float4 p = s_ctp[c], n4 = s_ctn[c];
        const float r[3] = {p.x - x[0], p.y - x[1], p.z - x[2]};
        const float n[3] = {n4.x, n4.y, n4.z};
        float tg = fdv((-p.w) * P.erp, P.dt);
        if (tg < 0.f) tg = 0.f;
        row_build(s_rows[c], r, n, Iw, tg);
        float t1[3], t2[3];
        plane_space(n, t1, t2);
        row_build(s_rows[MAXC + 2 * c], r, t1, Iw, 0.f);
        row_build(s_rows[MAXC + 2 * c + 1], r, t2, Iw, 0.f);
      }
      for (int it = 0; it < P.iterations; ++it) {
        for (int c = 0; c < nc; ++c) row_solve(s_rows[c], 0.f, INFINITY, v, w);
        for (int c = 0; c < nc; ++c) {
          const float lim = P.mu * s_rows[c].lambda;
          row_solve(s_rows[MAXC + 2 * c], -lim, lim, v, w);
          row_solve(s_rows[MAXC + 2 * c + 1], -lim, lim, v, w);
        }
      }
      float q[4] = {s_q[0], s_q[1], s_q[2], s_q[3]};
      for (int i = 0; i < 3; ++i) x[i] = x[i] + P.dt * v[i];
      const float o[4] = {(w[0] * q[3] + w[1] * q[2]) - w[2] * q[1], (w[1] * q[3] + w[2] * q[0]) - w[0] * q[2],
                          (w[2] * q[3] + w[0] * q[1]) - w[1] * q[0], -((w[0] * q[0] + w[1] * q[1]) + w[2] * q[2])};
      for (int i = 0; i < 4; ++i) q[i] = q[i] + P.half_dt * o[i];
      const float qn = fsq(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
      for (int i = 0; i < 4; ++i) s_q[i] = fdv(q[i], qn);
      for (int i = 0; i < 3; ++i) { s_x[i] = x[i]; s_v[i] = v[i]; s_w[i] = w[i]; }
      if (tr_state) {
        float* ts = tr_state + (size_t)step * TRACE_STATE;
        for (int i = 0; i < 3; ++i) ts[i] = s_x[i];
        for (int i = 0; i < 4; ++i) ts[3 + i] = s_q[i];
        for (int i = 0; i < 3; ++i) { ts[7 + i] = v[i]; ts[10 + i] = w[i]; }
        float* tc = tr_contacts + (size_t)step * MAXC * TRACE_CONTACT;
        for (int c = 0; c < nc; ++c) {
          const float4 p = s_ctp[c], n4 = s_ctn[c];
          const float e[8] = {p.x, p.y, p.z, n4.x, n4.y, n4.z, p.w, s_rows[c].lambda};
          for (int k = 0; k < 8; ++k) tc[c * TRACE_CONTACT + k] = e[k];
        }
        tr_n[step] = nc;
      }
    }
    __syncthreads();
  }

  if (tid == 0) {
    float R[9], W[16], O[16];
    R_from_q(s_q, R);
    for (int i = 0; i < 3; ++i) {
      for (int c = 0; c < 3; ++c) W[c * 4 + i] = R[3 * i + c];
      W[12 + i] = s_x[i];
      W[i * 4 + 3] = 0.f;
    }
    W[15] = 1.f;
    if (P.has_cam) mat4_mul(P.cam_inv, W, O);
    else
      for (int e = 0; e < 16; ++e) O[e] = W[e];
    for (int e = 0; e < 16; ++e) T_out[(size_t)st * 16 + e] = O[e];
    if (info) {
      pgp_physics_info inf;
      const int nc = s_nct;
      float md = 0.f;
      for (int c = 0; c < nc; ++c) md = fminf(md, s_ctp[c].w);
      inf.n_contacts = nc;
      inf.min_depth = md;
      inf.lin_speed = fsq(norm2_3(s_v[0], s_v[1], s_v[2]));
      inf.ang_speed = fsq(norm2_3(s_w[0], s_w[1], s_w[2]));
      info[st] = inf;
    }
  }
}

}  // namespace

namespace pgp {
namespace {

// ---- host: convex hull (double)------------------------------------------------------------------------------------
struct V3 {
  double x, y, z;
};
V3 sub(const V3& a, const V3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 crs(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dt3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
double len(const V3& a) { return std::sqrt(dt3(a, a)); }

struct Face {
  int a, b, c;
  V3 n;   // unit outward normal
  double d;
  bool alive;
};

Face make_face(const std::vector<V3>& P, int a, int b, int c) {
  Face f{a, b, c, {0, 0, 0}, 0, true};
  V3 n = crs(sub(P[b], P[a]), sub(P[c], P[a]));
  const double l = len(n);
  if (l > 0) n = {n.x / l, n.y / l, n.z / l};
  f.n = n;
  f.d = dt3(n, P[a]);
  return f;
}

// the hull of P[ids] (incremental, ids visited in order); false when degenerate.  faces: alive triangles
bool hull_faces(const std::vector<V3>& P, const std::vector<int>& ids, double eps, std::vector<Face>& faces) {
  faces.clear();
  if (ids.size() < 4) return false;
  // initial simplex: the smallest x (ties: first), the farthest from it, the farthest from their line, the farthest
  // from their plane (ties: first in ids order)
  int i0 = ids[0];
  for (int id : ids)
    if (P[id].x < P[i0].x) i0 = id;
  int i1 = -1;
  double best = -1;
  for (int id : ids) {
    const double d = dt3(sub(P[id], P[i0]), sub(P[id], P[i0]));
    if (d > best) { best = d; i1 = id; }
  }
  if (best <= eps * eps) return false;
  const V3 e01 = sub(P[i1], P[i0]);
  int i2 = -1;
  best = -1;
  for (int id : ids) {
    const double d = len(crs(e01, sub(P[id], P[i0]))) / len(e01);
    if (d > best) { best = d; i2 = id; }
  }
  if (best <= eps) return false;
  Face base = make_face(P, i0, i1, i2);
  int i3 = -1;
  best = -1;
  for (int id : ids) {
    const double d = std::fabs(dt3(base.n, P[id]) - base.d);
    if (d > best) { best = d; i3 = id; }
  }
  if (best <= eps) return false;
  if (dt3(base.n, P[i3]) - base.d > 0) std::swap(i1, i2);   // the apex lies below the base
  faces.push_back(make_face(P, i0, i1, i2));
  faces.push_back(make_face(P, i0, i3, i1));
  faces.push_back(make_face(P, i1, i3, i2));
  faces.push_back(make_face(P, i2, i3, i0));
  for (int id : ids) {
    if (id == i0 || id == i1 || id == i2 || id == i3) continue;
    std::set<std::pair<int, int>> edges;
    bool any = false;
    for (Face& f : faces)
      if (f.alive && dt3(f.n, P[id]) - f.d > eps) {
        f.alive = false;
        any = true;
        edges.insert({f.a, f.b});
        edges.insert({f.b, f.c});
        edges.insert({f.c, f.a});
      }
    if (!any) continue;
    for (const auto& e : edges)
      if (!edges.count({e.second, e.first})) faces.push_back(make_face(P, e.first, e.second, id));
    size_t k = 0;
    for (size_t i = 0; i < faces.size(); ++i)
      if (faces[i].alive) faces[k++] = faces[i];
    faces.resize(k);
  }
  return true;
}

}  // namespace

int convex_hull_impl(const float* xyz, int n, int max_vertices, std::vector<int>& hv, std::vector<std::array<double, 4>>& pl,
                     const char* who, std::vector<int4>* edges, std::vector<int>* loop_off, std::vector<int>* loop_idx) {
  if (!xyz || n < 4 || max_vertices < 4 || max_vertices > MAXV) {
    set_error("%s: bad argument (n = %d, max_vertices = %d of 4 .. %d)", who, n, max_vertices, MAXV);
    return PGP_EINVAL;
  }
  std::vector<V3> P(n);
  double scale = 0;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) {
      set_error("%s: point %d is not finite", who, i);
      return PGP_EINVAL;
    }
    P[i] = {p[0], p[1], p[2]};
    scale = std::max({scale, std::fabs(P[i].x), std::fabs(P[i].y), std::fabs(P[i].z)});
  }
  const double eps = 1e-7 * scale;
  std::vector<int> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = i;
  std::vector<Face> faces;
  for (int pass = 0; pass < 2; ++pass) {
    if (!hull_faces(P, ids, eps, faces)) {
      set_error("%s: degenerate input (no 4 points span a volume)", who);
      return PGP_EINVAL;
    }
    std::set<int> vs;
    for (const Face& f : faces) { vs.insert(f.a); vs.insert(f.b); vs.insert(f.c); }
    hv.assign(vs.begin(), vs.end());
    if ((int)hv.size() <= max_vertices) break;
    // farthest-point selection among the hull vertices, then the hull of the kept ones
    std::vector<double> dmin(hv.size(), INFINITY);
    std::vector<int> kept;
    size_t cur = 0;
    for (size_t i = 1; i < hv.size(); ++i)
      if (P[hv[i]].x > P[hv[cur]].x) cur = i;
    for (int k = 0; k < max_vertices; ++k) {
      kept.push_back(hv[cur]);
      dmin[cur] = -1;
      size_t nxt = 0;
      double bd = -2;
      for (size_t i = 0; i < hv.size(); ++i) {
        if (dmin[i] < 0) continue;
        const V3 d = sub(P[hv[i]], P[hv[cur]]);
        dmin[i] = std::min(dmin[i], dt3(d, d));
        if (dmin[i] > bd) { bd = dmin[i]; nxt = i; }
      }
      cur = nxt;
    }
    std::sort(kept.begin(), kept.end());
    ids = kept;
  }
  // coplanar triangles -> one plane: normal = the normalised sum of the group's area vectors, d = max over the hull
  std::vector<int> grp(faces.size(), -1);
  pl.clear();
  for (size_t i = 0; i < faces.size(); ++i) {
    if (grp[i] >= 0) continue;
    const Face& f = faces[i];
    V3 s{0, 0, 0};
    for (size_t j = i; j < faces.size(); ++j) {
      if (grp[j] >= 0) continue;
      const Face& g = faces[j];
      if (dt3(g.n, f.n) <= 0) continue;
      if (std::fabs(dt3(f.n, P[g.a]) - f.d) > eps || std::fabs(dt3(f.n, P[g.b]) - f.d) > eps ||
          std::fabs(dt3(f.n, P[g.c]) - f.d) > eps)
        continue;
      grp[j] = (int)pl.size();
      const V3 a = crs(sub(P[g.b], P[g.a]), sub(P[g.c], P[g.a]));
      s = {s.x + a.x, s.y + a.y, s.z + a.z};
    }
    const double l = len(s);
    const V3 nn = l > 0 ? V3{s.x / l, s.y / l, s.z / l} : f.n;
    double d = -INFINITY;
    for (int v : hv) d = std::max(d, dt3(nn, P[v]));
    pl.push_back({nn.x, nn.y, nn.z, d});
  }
  if (edges) {
    // hull edges from the topology: a triangle side shared by two triangles of different planes; the map orders
    // them by (v0, v1), v the position in hv
    edges->clear();
    std::map<std::pair<int, int>, std::pair<int, int>> em;   // (v0, v1) -> the planes of the two triangles
    for (size_t i = 0; i < faces.size(); ++i) {
      const int t[3] = {faces[i].a, faces[i].b, faces[i].c};
      for (int k = 0; k < 3; ++k) {
        const int va = (int)(std::lower_bound(hv.begin(), hv.end(), t[k]) - hv.begin());
        const int vb = (int)(std::lower_bound(hv.begin(), hv.end(), t[(k + 1) % 3]) - hv.begin());
        auto it = em.find({std::min(va, vb), std::max(va, vb)});
        if (it == em.end()) em[{std::min(va, vb), std::max(va, vb)}] = {grp[i], -1};
        else it->second.second = grp[i];
      }
    }
    for (const auto& e : em) {
      const int f0 = e.second.first, f1 = e.second.second;
      if (f1 < 0 || f0 == f1) continue;
      edges->push_back(make_int4(e.first.first, e.first.second, std::min(f0, f1), std::max(f0, f1)));
    }
  }
  if (loop_off && loop_idx) {
    // face loops from the topology: the triangles run counter-clockwise seen from outside, so a directed side whose
    // reverse belongs to a triangle of another plane is a side of its plane's loop, in loop direction
    loop_off->assign(1, 0);
    loop_idx->clear();
    const auto pos = [&](int v) { return (int)(std::lower_bound(hv.begin(), hv.end(), v) - hv.begin()); };
    std::map<std::pair<int, int>, int> side;   // directed (va, vb) -> the plane of its triangle
    for (size_t i = 0; i < faces.size(); ++i) {
      const int t[3] = {pos(faces[i].a), pos(faces[i].b), pos(faces[i].c)};
      for (int k = 0; k < 3; ++k) side[{t[k], t[(k + 1) % 3]}] = grp[i];
    }
    std::vector<std::map<int, int>> next(pl.size());
    for (const auto& s : side) {
      const auto rev = side.find({s.first.second, s.first.first});
      if (rev == side.end() || rev->second != s.second) next[s.second][s.first.first] = s.first.second;
    }
    for (const auto& nx : next) {
      if (!nx.empty()) {
        const int first = nx.begin()->first;   // the lowest vertex index of the loop
        int v = first;
        for (size_t k = 0; k < nx.size(); ++k) {
          loop_idx->push_back(v);
          const auto it = nx.find(v);
          if (it == nx.end()) break;
          v = it->second;
        }
      }
      loop_off->push_back((int)loop_idx->size());
    }
  }
  return PGP_OK;
}

int arena_upload(pgp_ctx* ctx) {
  int rc;
  if ((rc = ctx->d_phys_shapes.ensure(ctx->phys_shapes.size() * sizeof(PhysShape))) != PGP_OK) return rc;
  if ((rc = ctx->d_phys_verts.ensure(ctx->phys_verts.size() * sizeof(float4))) != PGP_OK) return rc;
  if ((rc = ctx->d_phys_planes.ensure(ctx->phys_planes.size() * sizeof(float4))) != PGP_OK) return rc;
  if ((rc = ctx->d_phys_eslices.ensure(ctx->phys_eslices.size() * sizeof(PhysEdgeSlice))) != PGP_OK) return rc;
  if ((rc = ctx->d_phys_edges.ensure(ctx->phys_edges.size() * sizeof(int4))) != PGP_OK) return rc;
  if ((rc = ctx->d_phys_fslices.ensure(ctx->phys_fslices.size() * sizeof(PhysFaceSlice))) != PGP_OK) return rc;
  if ((rc = ctx->d_phys_face_off.ensure(ctx->phys_face_off.size() * sizeof(int))) != PGP_OK) return rc;
  if ((rc = ctx->d_phys_face_idx.ensure(ctx->phys_face_idx.size() * sizeof(int))) != PGP_OK) return rc;
  PGP_HIP(hipMemcpy(ctx->d_phys_shapes.p, ctx->phys_shapes.data(), ctx->phys_shapes.size() * sizeof(PhysShape),
                    hipMemcpyHostToDevice));
  PGP_HIP(hipMemcpy(ctx->d_phys_verts.p, ctx->phys_verts.data(), ctx->phys_verts.size() * sizeof(float4), hipMemcpyHostToDevice));
  PGP_HIP(hipMemcpy(ctx->d_phys_planes.p, ctx->phys_planes.data(), ctx->phys_planes.size() * sizeof(float4),
                    hipMemcpyHostToDevice));
  PGP_HIP(hipMemcpy(ctx->d_phys_eslices.p, ctx->phys_eslices.data(), ctx->phys_eslices.size() * sizeof(PhysEdgeSlice),
                    hipMemcpyHostToDevice));
  PGP_HIP(hipMemcpy(ctx->d_phys_edges.p, ctx->phys_edges.data(), ctx->phys_edges.size() * sizeof(int4), hipMemcpyHostToDevice));
  PGP_HIP(hipMemcpy(ctx->d_phys_fslices.p, ctx->phys_fslices.data(), ctx->phys_fslices.size() * sizeof(PhysFaceSlice),
                    hipMemcpyHostToDevice));
  PGP_HIP(hipMemcpy(ctx->d_phys_face_off.p, ctx->phys_face_off.data(), ctx->phys_face_off.size() * sizeof(int), hipMemcpyHostToDevice));
  PGP_HIP(hipMemcpy(ctx->d_phys_face_idx.p, ctx->phys_face_idx.data(), ctx->phys_face_idx.size() * sizeof(int), hipMemcpyHostToDevice));
  return PGP_OK;
}

// appends a shape to the host mirror; the radius and inertia follow the rules of include/pgp.h
void arena_append(pgp_ctx* ctx, const std::vector<float4>& v, const std::vector<float4>& p, const std::vector<int4>& e,
                  const std::vector<int>& loop_off, const std::vector<int>& loop_idx, float margin) {
  PhysShape s{};
  s.vert_off = (int)ctx->phys_verts.size();
  s.n_vert = (int)v.size();
  s.plane_off = (int)ctx->phys_planes.size();
  s.n_plane = (int)p.size();
  s.margin = margin;
  double r = 0, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (const float4& a : v) {
    const double c[3] = {a.x, a.y, a.z};
    r = std::max(r, std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]));
    for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], c[i]); hi[i] = std::max(hi[i], c[i]); }
  }
  float rf = (float)r;
  if ((double)rf < r) rf = std::nextafter(rf, INFINITY);
  s.radius = rf;
  double l2[3];
  for (int i = 0; i < 3; ++i) {
    const double l = (hi[i] - lo[i]) + 6.0 * (double)margin;
    l2[i] = l * l;
  }
  s.inertia[0] = (float)((l2[1] + l2[2]) / 12.0);
  s.inertia[1] = (float)((l2[0] + l2[2]) / 12.0);
  s.inertia[2] = (float)((l2[0] + l2[1]) / 12.0);
  ctx->phys_shapes.push_back(s);
  ctx->phys_eslices.push_back(PhysEdgeSlice{(int)ctx->phys_edges.size(), (int)e.size()});
  ctx->phys_verts.insert(ctx->phys_verts.end(), v.begin(), v.end());
  ctx->phys_planes.insert(ctx->phys_planes.end(), p.begin(), p.end());
  ctx->phys_edges.insert(ctx->phys_edges.end(), e.begin(), e.end());
  ctx->phys_fslices.push_back(PhysFaceSlice{(int)ctx->phys_face_off.size(), (int)ctx->phys_face_idx.size()});
  ctx->phys_face_off.insert(ctx->phys_face_off.end(), loop_off.begin(), loop_off.end());
  ctx->phys_face_idx.insert(ctx->phys_face_idx.end(), loop_idx.begin(), loop_idx.end());
}

void arena_pop(pgp_ctx* ctx) {
  if (ctx->phys_shapes.empty()) return;
  ctx->phys_verts.resize(ctx->phys_shapes.back().vert_off);
  ctx->phys_planes.resize(ctx->phys_shapes.back().plane_off);
  ctx->phys_edges.resize(ctx->phys_eslices.back().edge_off);
  ctx->phys_face_off.resize(ctx->phys_fslices.back().off_off);
  ctx->phys_face_idx.resize(ctx->phys_fslices.back().idx_off);
  ctx->phys_shapes.pop_back();
  ctx->phys_eslices.pop_back();
  ctx->phys_fslices.pop_back();
}

int check_options(const pgp_physics_options* o, const char* who, int max_steps) {
  if (!o || !(o->dt > 0.f) || !std::isfinite(o->dt) || o->steps < 0 || o->steps > max_steps || o->iterations < 1 ||
      o->iterations > 1000 || !(o->linear_damping >= 0.f && o->linear_damping < 1.f) ||
      !(o->angular_damping >= 0.f && o->angular_damping < 1.f) || !(o->friction >= 0.f) || !std::isfinite(o->friction) ||
      !(o->erp >= 0.f && o->erp <= 1.f) || !std::isfinite(o->gravity[0]) || !std::isfinite(o->gravity[1]) ||
      !std::isfinite(o->gravity[2])) {
    set_error("%s: bad options", who);
    return PGP_EINVAL;
  }
  return PGP_OK;
}

static bool all_finite(const float* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

int make_params(pgp_ctx* ctx, const pgp_physics_options* o, int n_states, const float* table_params,
                const float* cam_pose, const char* who, PhysParams& P) {
  if (!table_params || !all_finite(table_params, 12) || (cam_pose && !all_finite(cam_pose, 16))) {
    set_error("%s: table_params missing or not finite, or cam_pose not finite", who);
    return PGP_EINVAL;
  }
  int rc = physics_arena_init(ctx);
  if (rc != PGP_OK) return rc;
  P = PhysParams{};
  P.n_states = n_states;
  P.steps = o->steps;
  P.iterations = o->iterations;
  P.n_shapes = (int)ctx->phys_shapes.size();
  P.dt = o->dt;
  P.half_dt = 0.5f * o->dt;
  P.w_max = HALF_PI_F / o->dt;
  P.lin_c = (float)std::pow(1.0 - (double)o->linear_damping, (double)o->dt);
  P.ang_c = (float)std::pow(1.0 - (double)o->angular_damping, (double)o->dt);
  P.mu = o->friction;
  P.erp = o->erp;
  for (int i = 0; i < 3; ++i) P.g[i] = o->gravity[i];
  for (int i = 0; i < 12; ++i) P.table[i] = table_params[i];
  P.has_cam = cam_pose != nullptr;
  if (cam_pose) {
    for (int i = 0; i < 16; ++i) P.cam[i] = cam_pose[i];
    // rigid inverse: R^T, -(R^T t)
    float* I = P.cam_inv;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) I[j * 4 + i] = cam_pose[i * 4 + j];
    for (int i = 0; i < 3; ++i)
      I[12 + i] = -((cam_pose[i * 4] * cam_pose[12] + cam_pose[i * 4 + 1] * cam_pose[13]) + cam_pose[i * 4 + 2] * cam_pose[14]);
    I[3] = I[7] = I[11] = 0.f;
    I[15] = 1.f;
  }
  return PGP_OK;
}

int launch_settle(pgp_ctx* ctx, const PhysParams& P, const int* d_dyn, const float* d_T, const int* d_off,
                  const int* d_ss, const float* d_sT, float* d_out, pgp_physics_info* d_info, float* tr_s, float* tr_c,
                  int* tr_n, hipStream_t st) {
  if (P.n_states == 0) return PGP_OK;
  // pgp_physics_set_polyhedral_contacts on: step 3p, whatever the edge switch says
  if (ctx->phys_poly_contacts) {
    hipLaunchKernelGGL(settle_poly_kernel, dim3(P.n_states), dim3(PT), 0, st, P, ctx->d_phys_shapes.as<PhysShape>(),
                       ctx->d_phys_verts.as<float4>(), ctx->d_phys_planes.as<float4>(), d_dyn, d_T, d_off, d_ss, d_sT, d_out,
                       d_info, tr_s, tr_c, tr_n, ctx->d_phys_eslices.as<PhysEdgeSlice>(), ctx->d_phys_edges.as<int4>(),
                       ctx->d_phys_fslices.as<PhysFaceSlice>(), ctx->d_phys_face_off.as<int>(), ctx->d_phys_face_idx.as<int>(),
                       ctx->phys_face_bias);
    PGP_HIP(hipGetLastError());
    return PGP_OK;
  }
  // the context's switch picks the instantiation (pgp_physics_set_edge_contacts); off: the vertex-face kernel
  auto* kernel = ctx->phys_edge_contacts ? settle_kernel<true> : settle_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(P.n_states), dim3(PT), 0, st, P, ctx->d_phys_shapes.as<PhysShape>(),
                     ctx->d_phys_verts.as<float4>(), ctx->d_phys_planes.as<float4>(), d_dyn, d_T, d_off, d_ss, d_sT, d_out,
                     d_info, tr_s, tr_c, tr_n, ctx->d_phys_eslices.as<PhysEdgeSlice>(), ctx->d_phys_edges.as<int4>(), ctx->phys_edge_reach);
  PGP_HIP(hipGetLastError());
  return PGP_OK;
}

// validates the host-side description of n states (shape ids, static ranges, finite poses)
int check_states(pgp_ctx* ctx, int n, const int* dyn, const float* T, const int* off, const int* ss, const float* sT,
                 const char* who) {
  const int ns = (int)ctx->phys_shapes.size();
  if (off[0] != 0) {
    set_error("%s: static_offsets[0] must be 0", who);
    return PGP_EINVAL;
  }
  for (int i = 0; i < n; ++i) {
    if (dyn[i] < 0 || dyn[i] >= ns) {
      set_error("%s: state %d names shape %d of %d", who, i, dyn[i], ns);
      return PGP_EINVAL;
    }
    if (off[i + 1] < off[i] || off[i + 1] - off[i] > PGP_PHYSICS_MAX_STATICS) {
      set_error("%s: state %d has %d statics (0 .. %d)", who, i, off[i + 1] - off[i], PGP_PHYSICS_MAX_STATICS);
      return PGP_EINVAL;
    }
    if (!all_finite(T + (size_t)i * 16, 16)) {
      set_error("%s: the pose of state %d is not finite", who, i);
      return PGP_EINVAL;
    }
  }
  const int m = off[n];
  if (m > 0 && (!ss || !sT)) {
    set_error("%s: statics without static_shape / static_T", who);
    return PGP_EINVAL;
  }
  for (int k = 0; k < m; ++k) {
    if (ss[k] < 0 || ss[k] >= ns) {
      set_error("%s: static %d names shape %d of %d", who, k, ss[k], ns);
      return PGP_EINVAL;
    }
    if (!all_finite(sT + (size_t)k * 16, 16)) {
      set_error("%s: the pose of static %d is not finite", who, k);
      return PGP_EINVAL;
    }
  }
  return PGP_OK;
}

int physics_arena_init(pgp_ctx* ctx) {
  if (!ctx->phys_shapes.empty()) return PGP_OK;
  // the table: btBoxShape(0.40, 0.40, 0.20) (PhySim.cpp:23), margin 0
  std::vector<float4> v, p;
  for (int i = 0; i < 8; ++i) v.push_back(make_float4(i & 1 ? 0.4f : -0.4f, i & 2 ? 0.4f : -0.4f, i & 4 ? 0.2f : -0.2f, 0.f));
  p = {make_float4(1, 0, 0, 0.4f), make_float4(-1, 0, 0, 0.4f), make_float4(0, 1, 0, 0.4f),
       make_float4(0, -1, 0, 0.4f), make_float4(0, 0, 1, 0.2f), make_float4(0, 0, -1, 0.2f)};
  // its 12 edges: vertices that differ in one bit; bit k set means the + side of axis k, planes 2k (+) and 2k + 1 (-)
  std::vector<int4> e;
  for (int i = 0; i < 8; ++i)
    for (int ax = 0; ax < 3; ++ax) {
      if (i & (1 << ax)) continue;
      const int o0 = ax == 0 ? 1 : 0, o1 = ax == 2 ? 1 : 2;
      e.push_back(make_int4(i, i | (1 << ax), 2 * o0 + (i & (1 << o0) ? 0 : 1), 2 * o1 + (i & (1 << o1) ? 0 : 1)));
    }
  std::sort(e.begin(), e.end(), [](const int4& a, const int4& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
  // its six quads, counter-clockwise seen from outside, each from its lowest vertex
  const std::vector<int> loop_off = {0, 4, 8, 12, 16, 20, 24};
  const std::vector<int> loop_idx = {1, 3, 7, 5, 0, 4, 6, 2, 2, 6, 7, 3, 0, 1, 5, 4, 4, 5, 7, 6, 0, 2, 3, 1};
  arena_append(ctx, v, p, e, loop_off, loop_idx, 0.f);
  const int rc = arena_upload(ctx);
  if (rc != PGP_OK) arena_pop(ctx);
  return rc;
}

}  // namespace pgp

