// tools/icp_plan_print.cc -- prints the launch plan of ICP calls (csrc/icp_plan.h) without a GPU: plain g++, no HIP.
//   g++ -std=c++17 -o icp_plan_print tools/icp_plan_print.cc
// One case per line on stdin, as key=value words; one line per case on stdout.  The steps are launch_icp's: validate,
// stage 1, the fit of the index stage 1 asked for, stage 2.
//   icp   n= n_src= n_tgt= n_cus= capturing= normals= scene_off= sum_block=       the shape
//         iters= trim= cap= ratio= metric= teps= rel= abs= drot= dtrans= smooth= nn_search=   pgp_icp_options (defaults:
//                                                                                 pgp_icp_default_options)
//         pose_fits= host_fits= lds=                                              the fit (default: neither index fits)
//         env.<field>=                                                            IcpEnv, by field name
//   multi jobs=n:n_src:ctx:fit[,...]  (fit: lds, l2 or none) + the options and env.<field> words
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../physimglobalpose_amd/csrc/icp_plan.h"

using namespace pgp;

static const char* form_name(IcpForm f) {
  switch (f) {
    case IcpForm::PerPose: return "per_pose";
    case IcpForm::Clustered: return "clustered";
    case IcpForm::Scene: return "scene";
    case IcpForm::Host: return "host";
    case IcpForm::Legacy: return "legacy";
  }
  return "?";
}
static const char* search_name(IcpSearch s) {
  switch (s) {
    case IcpSearch::Scan: return "scan";
    case IcpSearch::CappedGrid: return "capped_grid";
    case IcpSearch::OpenGrid: return "open_grid";
    case IcpSearch::IndexLds: return "index_lds";
    case IcpSearch::IndexL2: return "index_l2";
  }
  return "?";
}
static const char* want_name(IcpWant w) {
  switch (w) {
    case IcpWant::CappedGrid: return "capped_grid";
    case IcpWant::IndexPerPose: return "index_per_pose";
    case IcpWant::IndexHost: return "index_host";
    case IcpWant::NoIndex: return "no_index";
  }
  return "?";
}

static bool set_option(pgp_icp_options* o, const std::string& k, const char* v) {
  if (k == "iters") o->max_iterations = atoi(v);
  else if (k == "trim") o->trim_fraction = (float)atof(v);
  else if (k == "cap") o->max_corr_dist = (float)atof(v);
  else if (k == "ratio") o->energy_ratio = (float)atof(v);
  else if (k == "metric") o->error_metric = atoi(v);
  else if (k == "teps") o->transformation_epsilon = (float)atof(v);
  else if (k == "rel") o->relative_mse = (float)atof(v);
  else if (k == "abs") o->absolute_mse = (float)atof(v);
  else if (k == "drot") o->min_diff_rot = (float)atof(v);
  else if (k == "dtrans") o->min_diff_trans = (float)atof(v);
  else if (k == "smooth") o->smooth_length = atoi(v);
  else if (k == "nn_search") o->nn_search = atoi(v);
  else return false;
  return true;
}
static bool set_env(IcpEnv* e, const std::string& k, const char* v) {
#define PGP_FIELD(name, conv) \
  if (k == "env." #name) {    \
    e->name = conv;           \
    return true;              \
  }
  PGP_FIELD(nn, atoi(v)) PGP_FIELD(split, atoi(v)) PGP_FIELD(persist, atoi(v)) PGP_FIELD(scene_persist, atoi(v) != 0)
  PGP_FIELD(part, atoi(v) != 0) PGP_FIELD(open_grid, atoi(v) != 0) PGP_FIELD(multi, atoi(v) != 0)
  PGP_FIELD(wgs, atoi(v)) PGP_FIELD(image_global, atoi(v) != 0) PGP_FIELD(cell, atof(v)) PGP_FIELD(aspect, atof(v))
  PGP_FIELD(vic, atoi(v) != 0) PGP_FIELD(first_walk, atoi(v)) PGP_FIELD(solo_ticks, (unsigned)atoi(v)) PGP_FIELD(open_cell, atof(v))
  PGP_FIELD(scene_wgs, (unsigned)atoi(v)) PGP_FIELD(scene_sleep, atoi(v))
  PGP_FIELD(cooperative, atoi(v) != 0) PGP_FIELD(wait_ms, atof(v)) PGP_FIELD(force_lost, atoi(v) != 0)
  PGP_FIELD(debug, atoi(v) != 0)
#undef PGP_FIELD
  return false;
}
static pgp_icp_options default_options() {   // pgp_icp_default_options
  return pgp_icp_options{100, 1.f, 0.f, 1.f, 0, -1.f, 0.f, -1.f, 0.f, 0.f, 0, 0};
}

static int bad_word(const std::string& w) {
  printf("bad word %s\n", w.c_str());
  return 1;
}

static int icp_case(const std::vector<std::string>& words) {
  pgp_icp_options o = default_options();
  IcpEnv env;
  IcpShape s;
  bool pose_fits = false, host_fits = false, lds = false;
  for (const std::string& w : words) {
    const size_t eq = w.find('=');
    if (eq == std::string::npos) return bad_word(w);
    const std::string k = w.substr(0, eq);
    const char* v = w.c_str() + eq + 1;
    if (k == "n") s.n = atoi(v);
    else if (k == "n_src") s.n_src = atoi(v);
    else if (k == "n_tgt") s.n_tgt = atoi(v);
    else if (k == "n_cus") s.n_cus = atoi(v);
    else if (k == "capturing") s.capturing = atoi(v) != 0;
    else if (k == "normals") s.has_normals = atoi(v) != 0;
    else if (k == "scene_off") s.scene_form_off = atoi(v) != 0;
    else if (k == "sum_block") s.sum_block = atoi(v);
    else if (k == "pose_fits") pose_fits = atoi(v) != 0;
    else if (k == "host_fits") host_fits = atoi(v) != 0;
    else if (k == "lds") lds = atoi(v) != 0;
    else if (!set_option(&o, k, v) && !set_env(&env, k, v)) return bad_word(w);
  }
  const IcpError bad = icp_validate(&o, s);
  if (bad.rc != PGP_OK) return printf("rc=%s err=%s\n", bad.rc == PGP_EINVAL ? "EINVAL" : "?", bad.msg), 0;
  const IcpStage1 s1 = icp_stage1(&o, s, env);
  if (s1.err.rc != PGP_OK) return printf("rc=%s err=%s\n", s1.err.rc == PGP_EINVAL ? "EINVAL" : "?", s1.err.msg), 0;
  IcpFit fit;   // as launch_icp builds: the per-pose size first where stage 1 asks for it, then the host-driven size
  if (s1.want == IcpWant::IndexPerPose) fit.per_pose = pose_fits;
  if (s1.want == IcpWant::IndexHost || (s1.want == IcpWant::IndexPerPose && !fit.per_pose)) fit.host = host_fits;
  fit.image_in_lds = (fit.per_pose || fit.host) && lds;
  const IcpPlan p = icp_stage2(&o, s, env, s1, fit);
  if (p.err.rc != PGP_OK) return printf("rc=%s err=%s\n", p.err.rc == PGP_EINVAL ? "EINVAL" : "?", p.err.msg), 0;
  printf("rc=OK want=%s legacy=%d form=%s fallback=%s wgs=%d trim_only=%d pir=%d search=%s sums=%s n_blk=%d\n", want_name(s1.want),
         (int)s1.legacy, form_name(p.form), form_name(p.fallback), p.wgs_per_pose, (int)p.trim_only, p.pir, search_name(p.search),
         p.part_sums ? "block" : "whole", p.n_blk);
  return 0;
}

static int multi_case(const std::vector<std::string>& words) {
  pgp_icp_options o = default_options();
  IcpEnv env;
  std::vector<IcpMultiJob> jobs;
  std::vector<std::string> fits;
  static const char ctx_ids[64] = {0};   // contexts by number: distinct addresses
  for (const std::string& w : words) {
    const size_t eq = w.find('=');
    if (eq == std::string::npos) return bad_word(w);
    const std::string k = w.substr(0, eq);
    const char* v = w.c_str() + eq + 1;
    if (k == "jobs") {
      std::stringstream ss(v);
      std::string job;
      while (std::getline(ss, job, ',')) {
        int n = 0, n_src = 0, ctx = 0;
        char fit[16] = {0};
        if (sscanf(job.c_str(), "%d:%d:%d:%15s", &n, &n_src, &ctx, fit) != 4 || ctx < 0 || ctx >= 64) return bad_word(job);
        jobs.push_back(IcpMultiJob{n, n_src, ctx_ids + ctx});
        fits.push_back(fit);
      }
    } else if (!set_option(&o, k, v) && !set_env(&env, k, v)) return bad_word(w);
  }
  int built = 0;
  const IcpMultiPlan m = icp_multi_plan(&o, env, jobs.data(), (int)jobs.size(), [&](int j, int, int*) {
    ++built;
    return fits[(size_t)j] == "lds";
  });
  printf("one_launch=%d total=%d pir=%d trim_only=%d built=%d\n", (int)m.one_launch, m.total, m.pir, (int)m.trim_only, built);
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::stringstream ss(line);
    std::vector<std::string> words;
    std::string w;
    while (ss >> w) words.push_back(w);
    if (words.empty()) continue;
    const std::string kind = words[0];
    words.erase(words.begin());
    if (kind == "icp") icp_case(words);
    else if (kind == "multi") multi_case(words);
    else bad_word(kind);
  }
  return 0;
}
