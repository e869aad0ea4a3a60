// csrc/match_plan.h -- the host-side bookkeeping of the matcher's fit stage and chains: pure host code (no HIP; plain g++
// compiles it, tools/match_plan_check.cc and tests/test_match_plan_cpu.py pin it).  pgp_api.hip includes it.
#pragma once

#include <cstddef>
#include <vector>

namespace pgp {

void set_error(const char* fmt, ...);   // pgp_api.hip (the checker brings its own)

// The first n_bases successes (status 1, nothing else) among n_attempts attempts: their attempt numbers, in attempt order.
static inline std::vector<int> first_successes(const int* status, int n_attempts, int n_bases) {
  std::vector<int> kept;
  for (int a = 0; a < n_attempts && (int)kept.size() < n_bases; ++a)
    if (status[a] == 1) kept.push_back(a);
  return kept;
}

// The base of every pick: hb[4 k ..] = base_ids[4 * picks[2 k] ..] for the m picks (base, quad) -- hb may be pinned or not.
// nb >= 0: a pick that names a base outside [0, nb) ends the walk with `who`'s error text and false (the resident-batch
// calls, whose picks are the caller's).  nb < 0: unchecked (the chains, whose picks pgp_sample_quads drew over their own counts).
static inline bool pick_bases(const int* picks, size_t m, const int* base_ids, int* hb, int nb = -1, const char* who = "") {
  for (size_t k = 0; k < m; ++k) {
    const int b = picks[2 * k];
    if (nb >= 0 && (b < 0 || b >= nb)) {
      set_error("%s: pick %zu names base %d of %d", who, k, b, nb);
      return false;
    }
    for (int j = 0; j < 4; ++j) hb[4 * k + j] = base_ids[4 * (size_t)b + j];
  }
  return true;
}

// The lowest index of the maximum among the scores above 0 (a NaN is above nothing), and that score; none above 0: -1 and 0 --
// the verification loop's running best starts at 0 and takes strictly greater scores only (base.cc:1891-1908).
static inline int best_above_zero(const float* scores, int n, float* best_score) {
  int bi = -1;
  float bs = 0.f;
  for (int k = 0; k < n; ++k)
    if (scores[k] > bs) {
      bs = scores[k];
      bi = k;
    }
  *best_score = bs;
  return bi;
}

}  // namespace pgp
