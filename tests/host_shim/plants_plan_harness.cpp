// Compiles csrc/path_plan.h for the host (test infrastructure; tests/test_model_params_batch_host.py): the trailing `plants` argument of the
// path predicates — a handle that carries one set of model parameters per trajectory (to_set_model_params_batch).  (a) With the flag set,
// whatever the shape, traits and knobs: no scan, fused cooperative or fused lane step, whole candidates stored, one launch, one-wave
// workgroups, no repacked working set, and a report without fused / scan / working-set bits.  (b) Without it (argument left out, or false):
// every result equals what the predicates returned before the argument existed — `before` below is that code, kept verbatim.
#include "path_plan.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
using namespace to;

namespace before {
inline bool was_fused_coop_now(const PathPlan& p, int h_diag, int expand_variant) { return p.fused_coop && h_diag && (expand_variant == 0 || expand_variant == 2); }
inline bool was_scan_now(const PathPlan& p, int h_diag, int expand_variant) { return p.scan && was_fused_coop_now(p, h_diag, expand_variant) && expand_variant == 0; }
inline int was_roll_min(const PathPlan& p, const PathTraits& t) { return p.roll_min_active >= 0 ? p.roll_min_active : t.write_through ? 32768 : 2048; }
inline bool was_working_set_repack(const PathPlan& p, const PathTraits& t) { return p.fused_lane && p.compact && t.write_through && p.rp_min > 0; }
inline StepPlan was_plan_step(const PathPlan& p, const PathTraits& t, int h_diag, int expand_variant, int compact_armed, int last_active, int B) {
  StepPlan s;
  s.kind = p.fused_lane ? STEP_FUSED_LANE          // expansion in the registers of the lane that runs the recursion
           : was_scan_now(p, h_diag, expand_variant) && last_active <= p.scan_max_active ? STEP_SCAN  // the recursion as a scan over the horizon (k_scan.h)
           : was_fused_coop_now(p, h_diag, expand_variant) ? STEP_FUSED_COOP  // expansion by a second wave of the workgroup, through an LDS ring
           : STEP_SPLIT;
  const bool deep = p.cw_deep && last_active <= p.deep_max_active;
  s.CW = deep ? p.cw_deep : p.cw_base; s.TW = deep ? p.tw_deep : p.tw_base;
  s.two_wave = p.fwd2 == 2 && 2 * wave_blocks(last_active, s.TW) <= (long long)p.simds;
  const int rmin = was_roll_min(p, t);
  const bool dense = !t.write_through || (double)last_active >= p.roll_min_frac * (double)B;
  s.store_x = (rmin > 0 && t.accept_roll && !s.two_wave && last_active >= rmin && dense) ? 0 : 1;
  s.two_launch = !s.store_x && p.ls2_cwa && compact_armed && p.fwd2 != 1;
  return s;
}
inline void was_path_report(const PathPlan& p, const PathTraits& t, int h_diag, int expand_variant, int B, int32_t info[8]) {
  info[0] = p.bwd_mfma ? 1 : p.bwd_lane ? 2 : 0;
  info[1] = (p.fused_lane || was_fused_coop_now(p, h_diag, expand_variant)) ? 1 : 0;
  info[2] = p.compact;
  info[3] = p.cw_base;
  info[4] = (p.fwd2 && t.forward2) ? 2 : 1;  // (two-wave workgroups are used while the active trajectories leave room for them)
  info[5] = was_scan_now(p, h_diag, expand_variant) ? 1 : 0;
  info[6] = (t.accept_roll && p.roll_min_active != 0) ? 1 : 0;  // full-chip batch steps store candidate controls only (k_accept_roll)
  info[7] = p.repack_block0 != 0 ? 1 : 0;                        // repacked last line-search round
  if (was_working_set_repack(p, t) && B >= p.rp_min) info[7] |= 2;   // repacked working set (iLQR solves)
}
}  // namespace before

static long long fails = 0, checks = 0, flagged = 0, plain = 0, lane_handles = 0, mfma_handles = 0, compact_kept = 0, compact_dropped = 0;
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
// the models to_set_model_params_batch accepts, with the traits their launch tables report (models.h, ops_*.hip)
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
  // expand_variant as upload_tables derives it: bit 2 forced with the flag (7 with constraints or dense costs, 4 without)
  const int ev_plain = n_cons ? 2 : 0, ev_flag = ev_plain | 4;
  const int counts[] = {0, 1, 63, 64, 65, B / 4, B / 2, B - 1, B, p.deep_max_active, p.deep_max_active + 1, p.scan_max_active, 2047, 2048, 32767, 32768};
  for (int la : counts) {
    if (la < 0 || la > B) continue;
    for (int armed = 0; armed <= 1; ++armed) {
      // (a) flag set — with the variant the handle then has, and, for good measure, with the one it had before
      for (int ev : {ev_flag, ev_plain}) {
        const StepPlan s = plan_step(p, M.t, hd, ev, armed, la, B, true);
        ++flagged;
        CHECK(s.kind == STEP_SPLIT, "%s: %d active: step kind %d with per-trajectory model parameters", what, la, (int)s.kind);
        CHECK(s.store_x == 1 && !s.two_launch && !s.two_wave, "%s: %d active: store_x %d two_launch %d two_wave %d", what, la, s.store_x, (int)s.two_launch, (int)s.two_wave);
        CHECK(s.CW >= 1 && s.TW >= 1 && s.CW * s.TW <= 64, "%s: wave shape %d x %d", what, s.CW, s.TW);
      }
      // (b) no flag: what the predicates returned before the argument existed
      for (int ev : {ev_plain, ev_flag, 1, 3, 6}) {
        const StepPlan was = before::was_plan_step(p, M.t, hd, ev, armed, la, B);
        CHECK(same_step(plan_step(p, M.t, hd, ev, armed, la, B), was), "%s: %d active, variant %d: default argument changes the step", what, la, ev);
        CHECK(same_step(plan_step(p, M.t, hd, ev, armed, la, B, false), was), "%s: %d active, variant %d: plants = false changes the step", what, la, ev);
        ++plain;
      }
    }
  }
  for (int ev : {ev_plain, ev_flag, 1, 3, 6})
    for (int h : {0, 1}) {
      CHECK(!fused_coop_now(p, h, ev, true) && !scan_now(p, h, ev, true), "%s: fused / scan predicate with the flag", what);
      CHECK(fused_coop_now(p, h, ev) == before::was_fused_coop_now(p, h, ev) && fused_coop_now(p, h, ev, false) == before::was_fused_coop_now(p, h, ev), "%s: fused_coop_now", what);
      CHECK(scan_now(p, h, ev) == before::was_scan_now(p, h, ev) && scan_now(p, h, ev, false) == before::was_scan_now(p, h, ev), "%s: scan_now", what);
      int32_t a[8], b[8], c[8], f[8];
      path_report(p, M.t, h, ev, B, a); path_report(p, M.t, h, ev, B, b, false); before::was_path_report(p, M.t, h, ev, B, c);
      CHECK(!std::memcmp(a, c, sizeof a) && !std::memcmp(b, c, sizeof b), "%s: report without the flag differs", what);
      path_report(p, M.t, h, ev, B, f, true);
      CHECK(f[1] == 0 && f[5] == 0 && (f[7] & 2) == 0, "%s: report with the flag: fused %d scan %d working set %d", what, f[1], f[5], f[7]);
      CHECK(f[0] == c[0] && f[3] == c[3] && (f[7] & 1) == (c[7] & 1) && f[4] == 1 && f[6] == 0, "%s: report with the flag: flavour / width / rounds", what);
      CHECK(f[2] == solve_compact(p, true), "%s: report with the flag: compaction", what);
    }
  CHECK(!working_set_repack(p, M.t, true), "%s: working set with the flag", what);
  CHECK(working_set_repack(p, M.t) == before::was_working_set_repack(p, M.t) && working_set_repack(p, M.t, false) == before::was_working_set_repack(p, M.t), "%s: working_set_repack", what);
  // compaction: unchanged without the flag; with it only the MFMA path (whose kernels all take their trajectories from the list) keeps it
  CHECK(solve_compact(p) == p.compact && solve_compact(p, false) == p.compact, "%s: compaction without the flag", what);
  CHECK(solve_compact(p, true) == (p.bwd_mfma ? p.compact : 0), "%s: compaction with the flag", what);
  (solve_compact(p, true) ? compact_kept : compact_dropped) += 1;
}

int main() {
  const char* envs[] = {"", "BACKWARD=lane", "BACKWARD=coop", "BACKWARD=mfma", "SCAN=2", "SCAN=0", "FUSED_COOP=0", "FUSED_LANE=0", "FWD2=1", "FWD2=0", "ACCEPT_ROLL_MIN=1 ACCEPT_ROLL_FRAC=0",
                        "REPACK=64 BACKWARD=lane", "LS_TWO=1,4", "COMPACT=0", "LS_CANDIDATES=3", "EXPAND_LANE=0"};
  for (const Model& M : MODELS)
    for (int B : {1, 64, 70, 300, 1024, 12288, 32768, 70000})
      for (int N : {11, 31, 101, 201})
        for (int cons = 0; cons <= 2; cons += 2)
          for (int diag = 0; diag <= 1; ++diag)
            for (const char* env : envs) check(M, B, N, cons, diag != 0, env);
  printf("flagged %lld plain %lld lane_handles %lld mfma_handles %lld compact_kept %lld compact_dropped %lld\n", flagged, plain, lane_handles, mfma_handles, compact_kept, compact_dropped);
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
