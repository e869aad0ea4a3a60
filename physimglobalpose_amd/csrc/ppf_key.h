// csrc/ppf_key.h -- the point-pair feature of Match4PCSBase::computePPF (base.cc:582-598) and the device hash set
// of the model's feature table (pgp_set_ppf_map), shared by base selection (base_select.hip) and PPF voting
// (ppf_vote.hip): one statement of the key, so scene pairs of both use the table's exact convention.
#pragma once

#include "pgp_internal.h"
#include "exact_f32.h"

namespace pgp {
namespace ppfk {

using namespace exact;   // exact_f32.h: V3, ld3, vsub, cross, ...; the key and the base geometry sum as Eigen does (_eigen)

struct PpfTable {
  const unsigned long long* keys;  // open addressing, ~0ull = empty
  const uint32_t* value;           // key index (row of the CSR pair lists)
  uint32_t mask;
  int shift;
  float tpos[9], tneg[9];          // ratio thresholds of the 10-degree bins, x > 0 / x < 0
  int trans_disc;                  // 5 (mm)
};

__host__ __device__ inline int approximate_bin(int val, int disc) {  // base.cc:150-160
  const int lower = val - (val % disc), upper = lower + disc;
  return (val - lower < upper - val) ? lower : upper;
}

// approximate_bin(int(atan2f(y, x) * 180 / M_PI), 10) for y >= 0; -1 when the reference's value
// cannot be a table key (NaN inputs)
__device__ __forceinline__ int angle_bin(const PpfTable& t, float y, float x) {
  if (!(y == y) || !(x == x)) return -1;
  if (y == 0.f) return (__float_as_uint(x) >> 31) ? 180 : 0;   // atan2f(0, -0 or negative) = pi
  if (x == 0.f) return 90;
  const float r = __fdiv_rn(y, fabsf(x));
  int c = 0;
  if (x > 0.f) {
#pragma unroll
    for (int b = 0; b < 9; ++b) c += r >= t.tpos[b] ? 1 : 0;
    return 10 * c;
  }
#pragma unroll
  for (int b = 0; b < 9; ++b) c += r >= t.tneg[b] ? 1 : 0;
  return 180 - 10 * c;
}

// computePPF(i1, i2) packed as f1 << 24 | f2 << 16 | f3 << 8 | f4, or ~0ull when it is no key
__device__ __forceinline__ unsigned long long ppf_key(const PpfTable& t, V3 p1, V3 n1, V3 p2, V3 n2, int* f) {
  const V3 u = vsub(p1, p2);
  const int f1 = approximate_bin((int)mul(norm_eigen(u), 1000.0f), t.trans_disc);
  const int f2 = angle_bin(t, norm_eigen(cross(n1, u)), dot_eigen(n1, u));
  const int f3 = angle_bin(t, norm_eigen(cross(n2, u)), dot_eigen(n2, u));
  const int f4 = angle_bin(t, norm_eigen(cross(n1, n2)), dot_eigen(n1, n2));
  if (f) {
    f[0] = f1;
    f[1] = f2;
    f[2] = f3;
    f[3] = f4;
  }
  if (f1 < 0 || f2 < 0 || f3 < 0 || f4 < 0) return ~0ull;
  return ((unsigned long long)(unsigned)f1 << 24) | ((unsigned long long)f2 << 16) | ((unsigned long long)f3 << 8) |
         (unsigned long long)f4;
}

__device__ __forceinline__ int table_find(const PpfTable& t, unsigned long long key) {
  if (key == ~0ull || t.mask == 0u) return -1;
  uint32_t s = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> t.shift) & t.mask;
  for (;;) {   // load factor <= 0.5: an empty slot always ends the probe
    const unsigned long long k = t.keys[s];
    if (k == key) return (int)t.value[s];
    if (k == ~0ull) return -1;
    s = (s + 1) & t.mask;
  }
}

// the device view of the table pgp_set_ppf_map left in the context
inline void fill_ppf_table(const pgp_ctx* ctx, PpfTable* t) {
  t->keys = ctx->d_ppf_keys.as<unsigned long long>();
  t->value = ctx->d_ppf_val.as<uint32_t>();
  t->mask = ctx->ppf_mask;
  t->shift = ctx->ppf_shift;
  t->trans_disc = 5;   // base.cc:303
  std::memcpy(t->tpos, ctx->ppf_tpos, sizeof t->tpos);
  std::memcpy(t->tneg, ctx->ppf_tneg, sizeof t->tneg);
}

}  // namespace ppfk
}  // namespace pgp
