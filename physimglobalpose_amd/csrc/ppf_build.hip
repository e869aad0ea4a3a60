// csrc/ppf_build.hip -- the model's pair-feature table (PPFMap, PPE/data_layer/Objects.cpp:31-49) built on the device
// from the search model's points and normals, and installed as pgp_set_ppf_map installs the node's copy.
//
// The table: every ordered pair (i, j), i != j, filed under computePPF(i, j) (ppf_key.h, u = p_i - p_j), keys in
// std::map order (lexicographic = ascending packed key), pairs of a key in ascending (i, j) -- the order a double loop
// inserts them.  Both orders fall out of ONE radix sort of 64-bit composites
//     compact key << 2 ib | i << ib | j        (ib = bits of n - 1),
// compact key = f1 / 5 << 15 | f2 / 10 << 10 | f3 / 10 << 5 | f4 / 10 -- the features are multiples of their bins
// (approximate_bin), so the compact key orders as the feature vector does and the sort runs over
// 2 ib + 15 + bits(max f1 / 5) bits (n = 1000, a 30 cm object: 41 of 64).  No atomic decides a position: the pair pass
// writes composite (i, j) at i n + j, the sort is a key sort (equal keys are identical), boundaries are selected in
// order, so the table is bitwise the same from run to run.  Only the hash set's slot layout depends on the order of
// the compare-and-swaps, and no lookup can see it.
//
// Passes: pair pass (one composite per lane, the i-tile's points through LDS, coalesced 8-byte stores; invalid pairs
// and the diagonal ~0, which the sort leaves at the end) | rocprim::radix_sort_keys over the used bits, in a double
// buffer | rocprim::select of the key boundaries (a flag iterator over the sorted composites: no flag array) into
// the spare half of the double buffer = the CSR offsets | pair extraction | key decode + hash insert.
// Workspace: 2 x 8 n^2 bytes of composites + rocPRIM's scratch, freed before the call returns.

#include <cstring>  // rocprim's texture_cache_iterator.hpp uses memset without including it

#include "pgp_internal.h"
#include "ppf_key.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>

namespace pgp {

using namespace ppfk;

namespace {

constexpr int kTileJ = 256;   // columns of a pair-pass tile = threads of its workgroup
constexpr int kTileI = 16;    // rows of a tile: their points and normals sit in LDS
constexpr int kAngBits = 5;   // an angle bin / 10 is 0 .. 18
constexpr int kKeyLowBits = 3 * kAngBits;
// the widest model: pair distances up to 10 km keep f1 / 5 below 2^21, and 21 + 15 + 2 * 13 = 62 bits
constexpr int kMaxF1 = PGP_PPF_BUILD_MAX_MM + 5;

struct BuildStats {
  int max_f1;                   // largest distance key among the valid pairs (-1: none)
  int id_min, id_max;           // range of the ids in the pair lists
  int pad;
  unsigned long long n_valid;   // pairs that have a key
};

struct BuildTmp {   // transient device memory of one build
  void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~BuildTmp() {
    for (void* q : p)
      if (q) {
        hipError_t e = hipFree(q);
        (void)e;
      }
  }
  int alloc(int slot, size_t bytes) {
    hipError_t e = hipMalloc(&p[slot], std::max<size_t>(bytes, 16));
    if (e != hipSuccess) {
      p[slot] = nullptr;
      set_error("pgp_set_ppf_map_from_model: hipMalloc(%zu) of the build workspace failed: %s", bytes, hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? PGP_ENOMEM : PGP_EHIP;
    }
    return PGP_OK;
  }
};

__device__ __forceinline__ unsigned long long compact_key(const int* f) {
  return ((unsigned long long)(unsigned)(f[0] / 5) << kKeyLowBits) | ((unsigned long long)(f[1] / 10) << (2 * kAngBits)) |
         ((unsigned long long)(f[2] / 10) << kAngBits) | (unsigned long long)(f[3] / 10);
}

// composite (i, j) -> out[i n + j]; grid (ceil(n / kTileJ), ceil(n / kTileI))
__global__ __launch_bounds__(kTileJ) void ppf_build_pairs(PpfTable tab, const float4* __restrict__ P,
                                                          const float4* __restrict__ Nrm, int n, int ib,
                                                          unsigned long long* __restrict__ out, BuildStats* stats) {
  __shared__ float4 s_p[kTileI], s_n[kTileI];
  __shared__ int s_max_f1, s_id_min, s_id_max;
  __shared__ unsigned int s_valid;
  const int i0 = blockIdx.y * kTileI, j = blockIdx.x * kTileJ + threadIdx.x;
  if (threadIdx.x < kTileI && i0 + threadIdx.x < n) {
    s_p[threadIdx.x] = P[i0 + threadIdx.x];
    s_n[threadIdx.x] = Nrm[i0 + threadIdx.x];
  }
  if (threadIdx.x == 0) {
    s_max_f1 = -1;
    s_id_min = INT32_MAX;
    s_id_max = -1;
    s_valid = 0u;
  }
  __syncthreads();
  int max_f1 = -1, id_min = INT32_MAX, id_max = -1;
  unsigned int valid = 0u;
  if (j < n) {
    const float4 pj4 = P[j], nj4 = Nrm[j];
    const V3 pj = {pj4.x, pj4.y, pj4.z}, nj = {nj4.x, nj4.y, nj4.z};
    const int rows = min(kTileI, n - i0);
    for (int r = 0; r < rows; ++r) {
      const int i = i0 + r;
      unsigned long long c = ~0ull;
      if (i != j) {
        const float4 pi4 = s_p[r], ni4 = s_n[r];
        int f[4];
        const unsigned long long key = ppf_key(tab, {pi4.x, pi4.y, pi4.z}, {ni4.x, ni4.y, ni4.z}, pj, nj, f);
        if (key != ~0ull && f[0] <= kMaxF1) {   // (beyond: a non-finite distance, no key of any table)
          c = (compact_key(f) << (2 * ib)) | ((unsigned long long)i << ib) | (unsigned long long)j;
          max_f1 = max(max_f1, f[0]);
          id_min = min(id_min, min(i, j));
          id_max = max(id_max, max(i, j));
          ++valid;
        }
      }
      out[(size_t)i * (size_t)n + (size_t)j] = c;
    }
  }
  if (valid) {   // (maxima, minima and a count: the order of the atomics does not show)
    atomicMax(&s_max_f1, max_f1);
    atomicMin(&s_id_min, id_min);
    atomicMax(&s_id_max, id_max);
    atomicAdd(&s_valid, valid);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_valid) {
    atomicMax(&stats->max_f1, s_max_f1);
    atomicMin(&stats->id_min, s_id_min);
    atomicMax(&stats->id_max, s_id_max);
    atomicAdd(&stats->n_valid, (unsigned long long)s_valid);
  }
}

// 1 where a key's pair list starts in the sorted composites (the invalid tail never starts one)
struct KeyStart {
  const unsigned long long* sorted;
  int shift;
  __host__ __device__ bool operator()(uint32_t k) const {
    const unsigned long long c = sorted[k];
    if (c == ~0ull) return false;
    return k == 0u || (sorted[k - 1] >> shift) != (c >> shift);
  }
};

__global__ __launch_bounds__(256) void ppf_build_extract(const unsigned long long* __restrict__ sorted, uint32_t n_valid,
                                                         int ib, int2* __restrict__ pairs) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n_valid) return;
  const unsigned long long c = sorted[k];
  const unsigned int m = (1u << ib) - 1u;
  pairs[k] = make_int2((int)((unsigned int)(c >> ib) & m), (int)((unsigned int)c & m));
}

// row r: the packed key of its first pair into the open-addressing set (the hash and the probe of table_find), value = r
__global__ __launch_bounds__(256) void ppf_build_rows(const unsigned long long* __restrict__ sorted, uint32_t* __restrict__ off,
                                                      uint32_t n_keys, uint32_t n_valid, int ib, unsigned long long* tab_keys,
                                                      uint32_t* __restrict__ tab_val, uint32_t mask, int shift) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r == 0u) off[n_keys] = n_valid;
  if (r >= n_keys) return;
  const unsigned long long ck = sorted[off[r]] >> (2 * ib);
  const unsigned int a = (1u << kAngBits) - 1u;
  const unsigned long long f1 = (ck >> kKeyLowBits) * 5ull;
  const unsigned long long key = (f1 << 24) | ((unsigned long long)(((unsigned int)(ck >> (2 * kAngBits)) & a) * 10u) << 16) |
                                 ((unsigned long long)(((unsigned int)(ck >> kAngBits) & a) * 10u) << 8) |
                                 (unsigned long long)(((unsigned int)ck & a) * 10u);
  uint32_t s = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift) & mask;
  for (;;) {   // load factor <= 0.5 and distinct keys: an empty slot is always found
    if (atomicCAS(&tab_keys[s], ~0ull, key) == ~0ull) {
      tab_val[s] = r;
      return;
    }
    s = (s + 1) & mask;
  }
}

int bits_of(unsigned long long v) {
  int b = 0;
  while (v) {
    ++b;
    v >>= 1;
  }
  return b;
}

}  // namespace

int build_ppf_map(pgp_ctx* ctx, const float* xyz, const float* nrm, int n, int* n_keys_out, long long* n_pairs_out) {
  // the widest pair of finite points, in mm, must fit the distance field of the composite
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], (double)p[k]);
      hi[k] = std::max(hi[k], (double)p[k]);
    }
  }
  if (hi[0] >= lo[0]) {
    const double d[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double diag_mm = 1000.0 * std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(diag_mm <= (double)PGP_PPF_BUILD_MAX_MM)) {
      set_error("pgp_set_ppf_map_from_model: the model spans %.0f mm, more than PGP_PPF_BUILD_MAX_MM (%d)", diag_mm,
                PGP_PPF_BUILD_MAX_MM);
      return PGP_EINVAL;
    }
  }
  static_assert(kMaxF1 / 5 < (1 << 21), "the distance field of the composite");
  static_assert(PGP_PPF_BUILD_MAX_POINTS <= (1 << 13), "two ids and the compact key share 64 bits");

  // what the old table leaves behind goes first, as in set_ppf_map
  ctx->ppf_alpha_ready = false;
  ctx->csb_fit_m = 0;
  ctx->csb_nb = 0;
  int rc = ppf_thresholds(ctx->ppf_tpos, ctx->ppf_tneg);
  if (rc != PGP_OK) return rc;
  PpfTable tab{};
  tab.trans_disc = 5;   // base.cc:303
  std::memcpy(tab.tpos, ctx->ppf_tpos, sizeof tab.tpos);
  std::memcpy(tab.tneg, ctx->ppf_tneg, sizeof tab.tneg);

  hipStream_t st = ctx->stream;
  const size_t N = (size_t)n * (size_t)n;
  const int ib = std::max(1, bits_of((unsigned long long)(n - 1)));
  BuildTmp tmp;   // 0: points | normals, 1 / 2: the composites' double buffer, 3: rocPRIM scratch, 4: stats | key count
  if ((rc = tmp.alloc(0, (size_t)n * 32)) != PGP_OK || (rc = tmp.alloc(1, N * 8)) != PGP_OK ||
      (rc = tmp.alloc(2, N * 8)) != PGP_OK || (rc = tmp.alloc(4, sizeof(BuildStats) + 16)) != PGP_OK)
    return rc;
  float4* d_p = static_cast<float4*>(tmp.p[0]);
  float4* d_n = d_p + n;
  unsigned long long* buf0 = static_cast<unsigned long long*>(tmp.p[1]);
  unsigned long long* buf1 = static_cast<unsigned long long*>(tmp.p[2]);
  BuildStats* d_stats = static_cast<BuildStats*>(tmp.p[4]);
  unsigned int* d_count = reinterpret_cast<unsigned int*>(d_stats + 1);

  // the normals as pgp_set_scene stores them: as given
  std::vector<float4> h((size_t)2 * n);
  for (int i = 0; i < n; ++i) {
    h[i] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 0.f);
    h[(size_t)n + i] = make_float4(nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2], 0.f);
  }
  BuildStats hs{-1, INT32_MAX, -1, 0, 0ull};
  PGP_HIP(hipMemcpyAsync(d_p, h.data(), (size_t)n * 32, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemcpyAsync(d_stats, &hs, sizeof hs, hipMemcpyHostToDevice, st));
  PGP_HIP(hipMemsetAsync(d_count, 0, 16, st));
  hipLaunchKernelGGL(ppf_build_pairs, dim3((n + kTileJ - 1) / kTileJ, (n + kTileI - 1) / kTileI), dim3(kTileJ), 0, st, tab,
                     (const float4*)d_p, (const float4*)d_n, n, ib, buf0, d_stats);
  PGP_HIP(hipGetLastError());
  PGP_HIP(hipMemcpyAsync(&hs, d_stats, sizeof hs, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));

  const size_t n_valid = (size_t)hs.n_valid;
  if (n_valid == 0) {   // nothing has a key: the empty table
    if ((rc = set_ppf_map(ctx, nullptr, nullptr, nullptr, 0)) != PGP_OK) return rc;
    *n_keys_out = 0;
    *n_pairs_out = 0;
    return PGP_OK;
  }

  // the sort over the used bits only; the invalid composites (all ones) end up behind the valid ones
  const unsigned int end_bit = (unsigned int)(2 * ib + kKeyLowBits + std::max(1, bits_of((unsigned long long)(hs.max_f1 / 5))));
  rocprim::double_buffer<unsigned long long> db(buf0, buf1);
  size_t sort_bytes = 0, sel_bytes = 0;
  hipError_t he = rocprim::radix_sort_keys(nullptr, sort_bytes, db, N, 0u, end_bit, st);
  if (he != hipSuccess) {
    set_error("rocprim::radix_sort_keys (size query) failed: %s", hipGetErrorString(he));
    return PGP_EHIP;
  }
  const rocprim::counting_iterator<uint32_t> count_it(0u);
  he = rocprim::select(nullptr, sel_bytes, count_it, rocprim::make_transform_iterator(count_it, KeyStart{buf0, 2 * ib}),
                       (uint32_t*)nullptr, d_count, N, st);
  if (he != hipSuccess) {
    set_error("rocprim::select (size query) failed: %s", hipGetErrorString(he));
    return PGP_EHIP;
  }
  if ((rc = tmp.alloc(3, std::max(sort_bytes, sel_bytes))) != PGP_OK) return rc;
  he = rocprim::radix_sort_keys(tmp.p[3], sort_bytes, db, N, 0u, end_bit, st);
  if (he != hipSuccess) {
    set_error("rocprim::radix_sort_keys failed: %s", hipGetErrorString(he));
    return PGP_EHIP;
  }
  const unsigned long long* sorted = db.current();
  uint32_t* d_starts = reinterpret_cast<uint32_t*>(db.alternate());   // (N * 8 bytes: room for a start per composite)
  he = rocprim::select(tmp.p[3], sel_bytes, count_it, rocprim::make_transform_iterator(count_it, KeyStart{sorted, 2 * ib}),
                       d_starts, d_count, N, st);
  if (he != hipSuccess) {
    set_error("rocprim::select failed: %s", hipGetErrorString(he));
    return PGP_EHIP;
  }
  unsigned int n_keys = 0;
  PGP_HIP(hipMemcpyAsync(&n_keys, d_count, 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  if (n_keys == 0 || (size_t)n_keys > n_valid) {
    set_error("pgp_set_ppf_map_from_model: %u keys for %zu pairs", n_keys, n_valid);
    return PGP_EHIP;
  }

  // install: from here on the old table is gone
  ctx->ppf_ready = false;
  uint32_t size = 16;
  int lg = 4;
  while (size < 2u * n_keys) {
    size <<= 1;
    ++lg;
  }
  if ((rc = ctx->d_ppf_keys.ensure((size_t)size * 8)) != PGP_OK) return rc;
  if ((rc = ctx->d_ppf_val.ensure((size_t)size * 4)) != PGP_OK) return rc;
  if ((rc = ctx->d_ppf_off.ensure(((size_t)n_keys + 1) * 4)) != PGP_OK) return rc;
  if ((rc = ctx->d_ppf_pairs.ensure(n_valid * 8)) != PGP_OK) return rc;
  PGP_HIP(hipMemsetAsync(ctx->d_ppf_keys.p, 0xFF, (size_t)size * 8, st));
  PGP_HIP(hipMemsetAsync(ctx->d_ppf_val.p, 0, (size_t)size * 4, st));
  PGP_HIP(hipMemcpyAsync(ctx->d_ppf_off.p, d_starts, (size_t)n_keys * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(ppf_build_extract, dim3((unsigned int)((n_valid + 255) / 256)), dim3(256), 0, st, sorted,
                     (uint32_t)n_valid, ib, ctx->d_ppf_pairs.as<int2>());
  hipLaunchKernelGGL(ppf_build_rows, dim3((n_keys + 255u) / 256u), dim3(256), 0, st, sorted, ctx->d_ppf_off.as<uint32_t>(),
                     (uint32_t)n_keys, (uint32_t)n_valid, ib, ctx->d_ppf_keys.as<unsigned long long>(),
                     ctx->d_ppf_val.as<uint32_t>(), size - 1, 64 - lg);
  PGP_HIP(hipGetLastError());
  ctx->ppf_off_host.resize((size_t)n_keys + 1);
  PGP_HIP(hipMemcpyAsync(ctx->ppf_off_host.data(), ctx->d_ppf_off.p, ((size_t)n_keys + 1) * 4, hipMemcpyDeviceToHost, st));
  PGP_HIP(hipStreamSynchronize(st));
  ctx->ppf_mask = size - 1;
  ctx->ppf_shift = 64 - lg;
  ctx->ppf_n_keys = (int)n_keys;
  ctx->ppf_n_pairs = (long long)n_valid;
  ctx->ppf_has_pairs = true;
  ctx->ppf_id_min = hs.id_min;
  ctx->ppf_id_max = hs.id_max;
  ctx->ppf_max_f1 = hs.max_f1;
  ctx->ppf_ready = true;
  ctx->ppf_alpha_ready = false;
  *n_keys_out = (int)n_keys;
  *n_pairs_out = (long long)n_valid;
  return ppf_model_angles(ctx);
}

// The installed table in pgp_set_ppf_map's layout.  The key of a row is read out of the hash set (value = row); a row
// that no slot names -- pgp_set_ppf_map was handed a repeated or an unreachable key -- comes back as {-1, -1, -1, -1}.
int get_ppf_map(pgp_ctx* ctx, int* keys, int* counts, int* pairs, int cap_keys, long long cap_pairs, int* n_keys_out,
                long long* n_pairs_out) {
  if (!ctx->ppf_ready) {
    set_error("pgp_get_ppf_map: no pair-feature table (pgp_set_ppf_map / pgp_set_ppf_map_from_model first)");
    return PGP_ESTATE;
  }
  if (pairs && !ctx->ppf_has_pairs) {
    set_error("pgp_get_ppf_map: the table was set without its pair lists");
    return PGP_ESTATE;
  }
  const int n_keys = ctx->ppf_n_keys;
  const long long n_pairs = ctx->ppf_n_pairs;
  const int nk = std::min(n_keys, std::max(cap_keys, 0));
  hipStream_t st = ctx->stream;
  if (keys && nk > 0) {
    const size_t size = (size_t)ctx->ppf_mask + 1;
    std::vector<unsigned long long> tk(size);
    std::vector<uint32_t> tv(size);
    PGP_HIP(hipMemcpyAsync(tk.data(), ctx->d_ppf_keys.p, size * 8, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipMemcpyAsync(tv.data(), ctx->d_ppf_val.p, size * 4, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipStreamSynchronize(st));
    std::fill(keys, keys + 4 * (size_t)nk, -1);
    for (size_t s = 0; s < size; ++s) {
      if (tk[s] == ~0ull || tv[s] >= (uint32_t)nk) continue;
      int* f = keys + 4 * (size_t)tv[s];
      f[0] = (int)(tk[s] >> 24);
      f[1] = (int)((tk[s] >> 16) & 255u);
      f[2] = (int)((tk[s] >> 8) & 255u);
      f[3] = (int)(tk[s] & 255u);
    }
  }
  if (counts)
    for (int k = 0; k < nk; ++k) counts[k] = (int)(ctx->ppf_off_host[(size_t)k + 1] - ctx->ppf_off_host[k]);
  const long long np = std::min(n_pairs, std::max(cap_pairs, 0ll));
  if (pairs && np > 0) {
    PGP_HIP(hipMemcpyAsync(pairs, ctx->d_ppf_pairs.p, (size_t)np * 8, hipMemcpyDeviceToHost, st));
    PGP_HIP(hipStreamSynchronize(st));
  }
  *n_keys_out = n_keys;
  *n_pairs_out = n_pairs;
  return PGP_OK;
}

}  // namespace pgp
