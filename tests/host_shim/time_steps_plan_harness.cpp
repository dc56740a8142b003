// Compiles csrc/path_plan.h for the host (test infrastructure; tests/test_time_steps_host.py): a handle flagged for per-trajectory TIME STEPS
// (TableFlags::time_steps: DevProblem::dtb set, to_set_time_steps_batch) plans exactly what a handle flagged for per-trajectory PLANTS
// (TableFlags::plants, to_set_model_params_batch) plans — the same expansion variant for every combination of the other table flags, and, for
// every model / shape / knob row tests/host_shim/plants_plan_harness.cpp enumerates, the same step plan, report, compaction, working-set and
// forward-variant choice — and an unflagged handle plans what it planned before the flag existed.
#include "path_plan.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
using namespace to;

static long long fails = 0, checks = 0, steps = 0, reports = 0, variants = 0, lane_handles = 0, mfma_handles = 0, compact_kept = 0, compact_dropped = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static std::map<std::string, std::string> g_env;
static const char* lookup(const char* name) { auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }
static PathKnobs knobs(const char* env) {  // "NAME=value NAME=value" (names without the TRAJOPT_ prefix)
  g_env.clear();
  std::string s = env ? env : "";
  for (size_t i = 0; i < s.size();) {
    const size_t e = s.find('=', i), sp = s.find(' ', e) == std::string::npos ? s.size() : s.find(' ', e);
    g_env["TRAJOPT_" + s.substr(i, e - i)] = s.substr(e + 1, sp - e - 1);
    i = sp + 1;
  }
  return read_path_knobs(lookup);
}

struct Model { const char* name; int ne, m; PathTraits t; };
static PathTraits traits(bool wt, bool mfma, bool coop, bool lane, int ls, bool eb, bool ebc, bool ebs, bool ar, bool elk, bool ec, uint32_t f, uint32_t f2, uint32_t fp) {
  PathTraits t;
  t.write_through = wt; t.mfma_backward = mfma; t.coop_backward = coop; t.lane_backward = lane; t.ls_first_round = ls;
  t.expand_backward = eb; t.expand_backward_coop = ebc; t.expand_backward_scan = ebs; t.accept_roll = ar; t.expand_lane_k = elk; t.expand_const = ec;
  t.forward = f; t.forward2 = f2; t.forward_plants = fp;
  return t;
}
// the models to_set_time_steps_batch accepts (those of to_set_model_params_batch), with the traits their launch tables report (models.h, ops_*.hip)
static const Model MODELS[] = {
    {"double integrator 2", 4, 2, traits(true, false, true, true, 4, true, true, true, true, true, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"double integrator 3", 6, 3, traits(true, false, true, false, 4, false, false, false, true, false, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"cartpole", 4, 1, traits(true, true, true, true, 4, true, true, true, true, true, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"quadrotor", 12, 4, traits(false, true, false, false, 16, false, false, false, true, false, true, 0x0F0Fu | (3u << 18) | (3u << 26), 0x0F0Fu | (3u << 18) | (3u << 26), 0x0500u)},
};

static bool same_step(const StepPlan& a, const StepPlan& b) { return a.kind == b.kind && a.CW == b.CW && a.TW == b.TW && a.two_wave == b.two_wave && a.store_x == b.store_x && a.two_launch == b.two_launch; }

static void check(const Model& M, int B, int N, int n_cons, bool diag, const char* env) {
  PathShape sh;
  sh.B = B; sh.Bp = (B + 63) / 64 * 64; sh.N = N; sh.ne = M.ne; sh.m = M.m; sh.n_cons = n_cons; sh.diagonal_cost_blocks = diag;
  const PathPlan p = plan_paths(M.t, sh, knobs(env));
  const int hd = (!p.bwd_mfma && !p.bwd_lane && diag) ? 1 : 0;
  lane_handles += p.bwd_lane; mfma_handles += p.bwd_mfma;
  char what[200];
  snprintf(what, sizeof what, "%s B=%d N=%d cons=%d diag=%d [%s]", M.name, B, N, n_cons, (int)diag, env);
  TableFlags none, pl, ts, both;
  none.cons = pl.cons = ts.cons = both.cons = n_cons > 0;
  pl.plants = true; ts.time_steps = true; both.plants = both.time_steps = true;
  const bool r_pl = routed_as_plants(pl), r_ts = routed_as_plants(ts), r_both = routed_as_plants(both), r_none = routed_as_plants(none);
  CHECK(r_pl && r_ts && r_both && !r_none, "%s: routed_as_plants", what);
  const int ev_pl = expand_variant_of(pl), ev_ts = expand_variant_of(ts), ev_none = expand_variant_of(none);
  CHECK(ev_ts == ev_pl && expand_variant_of(both) == ev_pl && (ev_ts & 4) && ev_none == (n_cons ? 2 : 0), "%s: expansion variants %d %d %d", what, ev_pl, ev_ts, ev_none);
  const int counts[] = {0, 1, 63, 64, 65, B / 4, B / 2, B - 1, B, p.deep_max_active, p.deep_max_active + 1, p.scan_max_active, 2047, 2048, 32767, 32768};
  for (int la : counts) {
    if (la < 0 || la > B) continue;
    for (int armed = 0; armed <= 1; ++armed) {
      const StepPlan a = plan_step(p, M.t, hd, ev_pl, armed, la, B, r_pl), b = plan_step(p, M.t, hd, ev_ts, armed, la, B, r_ts);
      CHECK(same_step(a, b), "%s: %d active: a time-steps handle plans another step than a plants handle", what, la);
      CHECK(b.kind == STEP_SPLIT && b.store_x == 1 && !b.two_launch && !b.two_wave, "%s: %d active: kind %d store_x %d two_launch %d two_wave %d", what, la, (int)b.kind,
            b.store_x, (int)b.two_launch, (int)b.two_wave);
      ++steps;
    }
  }
  for (int h : {0, 1}) {
    int32_t a[8], b[8];
    path_report(p, M.t, h, ev_pl, B, a, r_pl); path_report(p, M.t, h, ev_ts, B, b, r_ts);
    CHECK(!std::memcmp(a, b, sizeof a), "%s: report of a time-steps handle differs from a plants handle's", what);
    CHECK(b[1] == 0 && b[5] == 0 && (b[7] & 2) == 0 && b[4] == 1 && b[6] == 0, "%s: report: fused %d scan %d working set %d", what, b[1], b[5], b[7]);
    CHECK(!fused_coop_now(p, h, ev_ts, r_ts) && !scan_now(p, h, ev_ts, r_ts), "%s: fused / scan predicate", what);
    ++reports;
  }
  CHECK(!working_set_repack(p, M.t, r_ts) && working_set_repack(p, M.t, r_ts) == working_set_repack(p, M.t, r_pl), "%s: working set", what);
  CHECK(solve_compact(p, r_ts) == solve_compact(p, r_pl) && solve_compact(p, r_ts) == (p.bwd_mfma ? p.compact : 0), "%s: compaction", what);
  (solve_compact(p, r_ts) ? compact_kept : compact_dropped) += 1;
  // the forward variant launch_forward picks for either handle: the general one-wave variant of the plants mask, never a SIMPLE one
  for (int rk4 = 0; rk4 <= 1; ++rk4) {
    const int mode = forward_mode(false, n_cons > 0, rk4 != 0, true, false, M.t.forward_plants);
    CHECK(mode >= 0 && (mode & 8) && !(mode & 1) && !(mode & 16), "%s: forward variant %d", what, mode);
  }
}

int main() {
  // every combination of the other table flags: the two flags give the same expansion variant, and without either nothing changed
  for (int bits = 0; bits < 32; ++bits) {
    TableFlags f;
    f.dense_costs = bits & 1; f.cons = bits & 2; f.non_selector = bits & 4; f.con_params = bits & 8; f.con_limits = bits & 16;
    const int was = (f.dense_costs ? 1 : 0) | (f.cons ? 2 : 0) | ((f.non_selector || f.con_params || f.con_limits) ? 4 : 0);
    TableFlags a = f, b = f;
    a.plants = true; b.time_steps = true;
    CHECK(expand_variant_of(f) == was, "flags %d: variant without either flag", bits);
    CHECK(expand_variant_of(a) == (was | 4) && expand_variant_of(b) == (was | 4), "flags %d: variant with a flag", bits);
    ++variants;
  }
  const char* envs[] = {"", "BACKWARD=lane", "BACKWARD=coop", "BACKWARD=mfma", "SCAN=2", "SCAN=0", "FUSED_COOP=0", "FUSED_LANE=0", "FWD2=1", "FWD2=0", "ACCEPT_ROLL_MIN=1 ACCEPT_ROLL_FRAC=0",
                        "REPACK=64 BACKWARD=lane", "LS_TWO=1,4", "COMPACT=0", "LS_CANDIDATES=3", "EXPAND_LANE=0"};
  for (const Model& M : MODELS)
    for (int B : {1, 64, 70, 300, 1024, 12288, 32768, 70000})
      for (int N : {11, 31, 101, 201})
        for (int cons = 0; cons <= 2; cons += 2)
          for (int diag = 0; diag <= 1; ++diag)
            for (const char* env : envs) check(M, B, N, cons, diag != 0, env);
  printf("steps %lld reports %lld variants %lld lane_handles %lld mfma_handles %lld compact_kept %lld compact_dropped %lld\n", steps, reports, variants, lane_handles, mfma_handles, compact_kept, compact_dropped);
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
