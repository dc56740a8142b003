// Compiles csrc/path_plan.h for the host (test infrastructure; tests/test_constraint_limits_host.py): how a handle whose constraints carry
// per-trajectory LIMITS (to_set_constraint_limits_batch, DevProblem::cl) is routed.  (a) Flagged: the variant, every step plan, the report and the
// forward-pass variant are those of the same handle with per-trajectory constraint PARAMETERS (DevProblem::cp) — bit 2 of the variant forced, so no
// scan step, no fused cooperative step, forward `mode | 8`.  (b) Unflagged, and again after the flag is cleared: the variant is what upload_tables
// computed before TableFlags existed (`before` below is that code, kept verbatim) and with it every plan is the one it is today.
#include "path_plan.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
using namespace to;

namespace before {
inline int was_expand_variant(bool dense, bool no_cons, bool non_selector, bool cp_flagged, bool pm) {
  bool generic = false;
  generic = generic || non_selector;
  generic = generic || cp_flagged;
  generic = generic || pm;
  return (dense ? 1 : 0) | (no_cons ? 0 : 2) | (generic ? 4 : 0);
}
inline bool was_forward_general(int expand_variant, bool gl, bool cp) { return (expand_variant & 5) || gl || cp; }
}  // namespace before

static long long fails = 0, checks = 0, flagged = 0, plain = 0, cleared = 0, scan_plain = 0, fused_plain = 0, lane_flagged = 0, two_wave_flagged = 0, repack_flagged = 0;
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
// the trait sets of models.h with the launchers the ops_*.hip translation units fill (as in path_plan_harness.cpp)
static const Model MODELS[] = {
    {"double integrator 2", 4, 2, traits(true, false, true, true, 4, true, true, true, true, true, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"double integrator 3", 6, 3, traits(true, false, true, false, 4, false, false, false, true, false, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"cartpole", 4, 1, traits(true, true, true, true, 4, true, true, true, true, true, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"quadrotor", 12, 4, traits(false, true, false, false, 16, false, false, false, true, false, true, 0x0F0Fu | (3u << 18) | (3u << 26), 0x0F0Fu | (3u << 18) | (3u << 26), 0x0500u)},
    {"quadrotor mrp/rp", 12, 4, traits(false, true, false, false, 16, false, false, false, true, false, true, (1u << 8) | (1u << 10), (1u << 8) | (1u << 10), 0u)},
    {"hybrid", 4, 2, traits(true, false, true, true, 4, true, true, true, true, true, false, 0xFFFFu, 0xFFFFu, 0u)},
};

static bool same_step(const StepPlan& a, const StepPlan& b) { return a.kind == b.kind && a.CW == b.CW && a.TW == b.TW && a.two_wave == b.two_wave && a.store_x == b.store_x && a.two_launch == b.two_launch; }

static void check(const Model& M, int B, int N, bool dense, bool non_selector, bool diag, const char* env) {
  PathShape sh;
  sh.B = B; sh.Bp = (B + 63) / 64 * 64; sh.N = N; sh.ne = M.ne; sh.m = M.m; sh.n_cons = 2; sh.diagonal_cost_blocks = diag;  // (limits need a constraint)
  const PathPlan p = plan_paths(M.t, sh, knobs(env));
  char what[200];
  snprintf(what, sizeof what, "%s B=%d N=%d dense=%d generic=%d diag=%d [%s]", M.name, B, N, (int)dense, (int)non_selector, (int)diag, env);
  TableFlags base;
  base.dense_costs = dense; base.cons = true; base.non_selector = non_selector;
  TableFlags lim = base, par = base, both = base;
  lim.con_limits = true; par.con_params = true; both.con_limits = both.con_params = true;
  const int ev0 = expand_variant_of(base), evl = expand_variant_of(lim), evp = expand_variant_of(par), evb = expand_variant_of(both);
  // (b) unflagged / cleared: today's variant
  CHECK(ev0 == before::was_expand_variant(dense, false, non_selector, false, false), "%s: unflagged variant %d", what, ev0);
  TableFlags again = lim; again.con_limits = false;  // to_clear_constraint_limits_batch / to_set_constraint on the last flagged constraint
  CHECK(expand_variant_of(again) == ev0, "%s: variant after clear %d, unflagged %d", what, expand_variant_of(again), ev0);
  ++cleared;
  // (a) flagged: the variant of the cp handle, bit 2 set, the other bits kept
  CHECK(evl == evp && evl == evb && evp == before::was_expand_variant(dense, false, non_selector, true, false), "%s: variants limits %d params %d both %d", what, evl, evp, evb);
  CHECK((evl & 4) && (evl & 3) == (ev0 & 3) && evl == (dense ? 7 : 6), "%s: flagged variant %d from %d", what, evl, ev0);
  // unconstrained tables (no constraint can be flagged), and plants
  TableFlags none; none.dense_costs = dense;
  CHECK(expand_variant_of(none) == before::was_expand_variant(dense, true, false, false, false), "%s: unconstrained variant", what);
  TableFlags pl = base; pl.plants = true;
  CHECK(expand_variant_of(pl) == before::was_expand_variant(dense, false, non_selector, false, true), "%s: plants variant", what);
  // h_diag as upload_tables derives it (the cost blocks stay diagonal: limits change no Jacobian)
  const int hd = (!p.bwd_mfma && !p.bwd_lane && diag) ? 1 : 0;
  const int counts[] = {0, 1, 63, 64, 65, B / 4, B / 2, B - 1, B, p.deep_max_active, p.deep_max_active + 1, p.scan_max_active, 2047, 2048, 32767, 32768};
  for (int la : counts) {
    if (la < 0 || la > B) continue;
    for (int armed = 0; armed <= 1; ++armed) {
      const StepPlan sl = plan_step(p, M.t, hd, evl, armed, la, B), sp = plan_step(p, M.t, hd, evp, armed, la, B), s0 = plan_step(p, M.t, hd, ev0, armed, la, B);
      ++flagged;
      CHECK(same_step(sl, sp), "%s: %d active: limits step differs from the parameters step", what, la);
      CHECK(sl.kind != STEP_SCAN && sl.kind != STEP_FUSED_COOP, "%s: %d active: step kind %d with per-trajectory limits", what, la, (int)sl.kind);
      // everything but the kind is decided without the variant: the flagged handle keeps the wave shape, the stores and the launches of today
      CHECK(sl.CW == s0.CW && sl.TW == s0.TW && sl.two_wave == s0.two_wave && sl.store_x == s0.store_x && sl.two_launch == s0.two_launch, "%s: %d active: shape / stores change with the flag", what, la);
      CHECK(sl.kind == s0.kind || s0.kind == STEP_SCAN || s0.kind == STEP_FUSED_COOP, "%s: %d active: kind %d -> %d", what, la, (int)s0.kind, (int)sl.kind);
      lane_flagged += sl.kind == STEP_FUSED_LANE; two_wave_flagged += sl.two_wave;
      scan_plain += s0.kind == STEP_SCAN; fused_plain += s0.kind == STEP_FUSED_COOP;
      ++plain;
    }
  }
  for (int h : {0, 1}) {
    CHECK(!fused_coop_now(p, h, evl) && !scan_now(p, h, evl), "%s: fused cooperative / scan predicate with the flag", what);
    int32_t a[8], b[8];
    path_report(p, M.t, h, evl, B, a); path_report(p, M.t, h, evp, B, b);
    CHECK(!std::memcmp(a, b, sizeof a), "%s: report with limits differs from the report with parameters", what);
    CHECK(a[5] == 0, "%s: report names the scan kernel", what);
    repack_flagged += (a[7] & 2) != 0;
  }
  // forward-pass variant: general for a flagged handle whatever the variant bits say, and the one of the cp handle; unflagged: today's request
  for (int simple = 0; simple <= 1; ++simple)
    for (int rk4 = 0; rk4 <= 1; ++rk4)
      for (int unit = 0; unit <= 1; ++unit)
        for (int gl = 0; gl <= 1; ++gl) {
          CHECK(forward_general(ev0, gl, false, true) && forward_general(evl, gl, false, true), "%s: forward pass not general with limits", what);
          const int ml = forward_mode(simple, true, rk4, forward_general(evl, gl, false, true), false, M.t.forward);     // (unit_soc is 0 while a cone is flagged)
          const int mp = forward_mode(simple, true, rk4, forward_general(evp, gl, true, false), false, M.t.forward);
          CHECK(ml == mp && (ml < 0 || (ml & 8)), "%s: forward variant %d with limits, %d with parameters", what, ml, mp);
          CHECK(forward_general(ev0, gl, false, false) == before::was_forward_general(ev0, gl, false), "%s: unflagged forward request", what);
          CHECK(forward_mode(simple, true, rk4, forward_general(ev0, gl, false, false), unit, M.t.forward) ==
                    forward_mode(simple, true, rk4, before::was_forward_general(ev0, gl, false), unit, M.t.forward), "%s: unflagged forward variant", what);
        }
}

int main() {
  const char* envs[] = {"", "BACKWARD=lane", "BACKWARD=lane ACCEPT_ROLL_MIN=1", "BACKWARD=coop", "BACKWARD=mfma", "SCAN=2", "SCAN=0", "FUSED_COOP=0", "FUSED_LANE=0", "FWD2=1", "FWD2=0",
                        "ACCEPT_ROLL_MIN=1 ACCEPT_ROLL_FRAC=0", "REPACK=64 BACKWARD=lane", "LS_TWO=1,4", "COMPACT=0", "LS_CANDIDATES=3", "EXPAND_LANE=0"};
  for (const Model& M : MODELS)
    for (int B : {1, 24, 40, 64, 70, 300, 1024, 8192, 12288, 32768, 70000})
      for (int N : {11, 51, 61, 101, 201})
        for (int dense = 0; dense <= 1; ++dense)
          for (int generic = 0; generic <= 1; ++generic)
            for (int diag = 0; diag <= 1; ++diag)
              for (const char* env : envs) check(M, B, N, dense != 0, generic != 0, diag != 0, env);
  printf("flagged %lld plain %lld cleared %lld scan_plain %lld fused_plain %lld lane_flagged %lld two_wave_flagged %lld repack_flagged %lld\n", flagged, plain, cleared, scan_plain,
         fused_plain, lane_flagged, two_wave_flagged, repack_flagged);
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
