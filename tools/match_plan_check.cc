// tools/match_plan_check.cc -- checks the matcher's host-side bookkeeping (csrc/match_plan.h) without a GPU: plain g++, no HIP.
//   g++ -std=c++17 -fsanitize=address,undefined -o match_plan_check tools/match_plan_check.cc && ./match_plan_check
// Prints one line per failed case and exits non-zero if there is one; the sanitizers watch the array accesses.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../physimglobalpose_amd/csrc/match_plan.h"

static char g_err[256] = "";
void pgp::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

using namespace pgp;

static int g_failed = 0;
static void expect(bool ok, const char* what) {
  if (ok) return;
  printf("FAILED: %s\n", what);
  ++g_failed;
}

static void compaction() {
  using V = std::vector<int>;
  expect(first_successes(nullptr, 0, 3).empty(), "compaction: 0 attempts");
  const V none = {0, 0, 0, 0};
  expect(first_successes(none.data(), 4, 3).empty(), "compaction: all failed");
  const V exact = {1, 0, 1, 0, 1};
  expect(first_successes(exact.data(), 5, 3) == V({0, 2, 4}), "compaction: exactly n_bases successes");
  const V more = {0, 1, 1, 0, 1, 1, 1};
  expect(first_successes(more.data(), 7, 3) == V({1, 2, 4}), "compaction: the surplus is ignored, order kept");
  expect(first_successes(more.data(), 7, 100) == V({1, 2, 4, 5, 6}), "compaction: fewer successes than n_bases");
  expect(first_successes(more.data(), 7, 0).empty(), "compaction: n_bases 0");
  const V odd = {2, -1, 1, 255, 0, 1, 3};
  expect(first_successes(odd.data(), 7, 5) == V({2, 5}), "compaction: only status 1 is a success");
}

static void picks() {
  const int nb = 3;
  const std::vector<int> ids = {10, 11, 12, 13, 20, 21, 22, 23, 30, 31, 32, 33};   // exactly 4 nb: one past the end is the sanitizer's
  {
    g_err[0] = 0;
    expect(pick_bases(nullptr, 0, ids.data(), nullptr, nb, "f") && !g_err[0], "pick_bases: m = 0");
    expect(pick_bases(nullptr, 0, ids.data(), nullptr), "pick_bases: m = 0, unchecked");
  }
  {
    const std::vector<int> pk = {2, 7, 0, 0, 2, 1};   // the last valid base, twice; the quad numbers are not read
    std::vector<int> hb(12, -7);
    g_err[0] = 0;
    expect(pick_bases(pk.data(), 3, ids.data(), hb.data(), nb, "f") && !g_err[0], "pick_bases: the last valid base");
    expect(hb == std::vector<int>({30, 31, 32, 33, 10, 11, 12, 13, 30, 31, 32, 33}), "pick_bases: the bases of the picks");
    std::vector<int> hb2(12, -7);
    expect(pick_bases(pk.data(), 3, ids.data(), hb2.data()) && hb2 == hb, "pick_bases: unchecked, same bases");
  }
  {
    const std::vector<int> pk = {1, 0, -1, 0, 2, 0};
    std::vector<int> hb(12, -7);
    g_err[0] = 0;
    expect(!pick_bases(pk.data(), 3, ids.data(), hb.data(), nb, "pgp_congruent_batch_fit"), "pick_bases: base -1 is refused");
    expect(!strcmp(g_err, "pgp_congruent_batch_fit: pick 1 names base -1 of 3"), "pick_bases: the text for base -1");
    expect(hb[3] == 23 && hb[4] == -7, "pick_bases: nothing written from the bad pick on");
  }
  {
    const std::vector<int> pk = {3, 0};
    std::vector<int> hb(4, -7);
    g_err[0] = 0;
    expect(!pick_bases(pk.data(), 1, ids.data(), hb.data(), nb, "pgp_congruent_batch_fit_score_list"), "pick_bases: base nb is refused");
    expect(!strcmp(g_err, "pgp_congruent_batch_fit_score_list: pick 0 names base 3 of 3"), "pick_bases: the text for base nb");
    expect(!pick_bases(pk.data(), 1, ids.data(), hb.data(), 0, "f"), "pick_bases: no batch resident, every pick is refused");
  }
}

static void best() {
  float bs = -1.f;
  expect(best_above_zero(nullptr, 0, &bs) == -1 && bs == 0.f, "best: empty");
  const std::vector<float> zeros = {0.f, 0.f, -0.f};
  bs = -1.f;
  expect(best_above_zero(zeros.data(), 3, &bs) == -1 && bs == 0.f, "best: all zeros");
  const std::vector<float> nan_first = {NAN, 0.25f, NAN, 0.5f, NAN};
  expect(best_above_zero(nan_first.data(), 5, &bs) == 3 && bs == 0.5f, "best: a NaN is never the best");
  const std::vector<float> nan_only = {NAN, NAN};
  expect(best_above_zero(nan_only.data(), 2, &bs) == -1 && bs == 0.f, "best: only NaNs");
  const std::vector<float> ties = {0.5f, 1.f, 0.75f, 1.f, 1.f};
  expect(best_above_zero(ties.data(), 5, &bs) == 1 && bs == 1.f, "best: ties at the top go to the lowest index");
  const float neg = -0.5f;
  expect(best_above_zero(&neg, 1, &bs) == -1 && bs == 0.f, "best: a single negative score");
  const float tiny = 1e-45f;   // the smallest denormal is above 0
  expect(best_above_zero(&tiny, 1, &bs) == 0 && bs == tiny, "best: strictly greater than 0 is enough");
}

int main() {
  compaction();
  picks();
  best();
  if (g_failed) return 1;
  printf("match_plan ok\n");
  return 0;
}
