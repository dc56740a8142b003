// Compiles the host-only side of per-trajectory cost weights as a program of its own (test infrastructure; tests/test_cost_weights_host.py,
// which builds it with -fsanitize=address,undefined as well): csrc/desc_lower.h — every refusal of to_set_cost_weights_batch / to_get_... /
// to_clear_... and of to_set_tracking_reference_batch on a handle with weights, the host copy and its tiling —, csrc/path_plan.h — how such a
// handle is routed — and csrc/rp_plan.h — the re-use rule of the repacked working set.  Prints
//   case <name> code <c> msg <text>     every refusal, with the error class and the message;
//   counts of the routing checks, then "checks <n> fails <n>".
#include "desc_lower.h"
#include "path_plan.h"
#include "rp_plan.h"

#include <cstdio>
#include <limits>
#include <string>
#include <vector>

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

static long long fails = 0, checks = 0, flagged = 0, plain = 0, lane_flagged = 0, two_wave_flagged = 0, repack_flagged = 0, fused_plain = 0, simple_plain = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static const int n = 4, m = 2, B = 70, Bp = 128, NC = 3;

static std::vector<to_cost_desc> costs(int kind2 = TO_COST_DIAGONAL) {
  std::vector<to_cost_desc> c(NC);
  for (int ci = 0; ci < NC; ++ci) {
    std::memset(&c[ci], 0, sizeof(to_cost_desc));
    c[ci].kind = ci == 2 ? kind2 : (ci == 1 ? TO_COST_DIAGONAL_QUAT : TO_COST_DIAGONAL);
    for (int i = 0; i < n; ++i) c[ci].Q[i] = 10.0 * (ci + 1) + i;
    for (int j = 0; j < m; ++j) c[ci].R[j] = 0.1 * (ci + 1) + 0.01 * j;
  }
  return c;
}
static CostWeightFacts facts(const std::vector<to_cost_desc>& c, int key = 3, bool in_flight = false, int Nref = 0) {
  static const char* names[] = {"double integrator (D = 1)", "double integrator (D = 2)", "double integrator (D = 3)", "Cartpole", "Quadrotor", "Quadrotor{MRP}",
                                "Quadrotor{RodriguesParam}", "hybrid double integrator", "model vector", "InfeasibleModel (double integrator, D = 1)",
                                "InfeasibleModel (double integrator, D = 2)", "InfeasibleModel (Cartpole)"};
  return CostWeightFacts{key, names[key], n, m, B, c.data(), (int)c.size(), in_flight, Nref};
}
static void report(const char* name, int rc) { printf("case %s code %d msg %s\n", name, rc, g_err.c_str()); g_err.clear(); }

static void refusals() {
  const auto c = costs();
  std::vector<double> Q((size_t)n * B, 1.0), R((size_t)m * B, 0.5);
  CostWeightFacts f = facts(c);
  CHECK(validate_cost_weights(&f, 0, Q.data(), R.data()) == TO_OK, "a plain call is accepted: %s", g_err.c_str());
  CHECK(validate_cost_weights(&f, 1, Q.data(), nullptr) == TO_OK && validate_cost_weights(&f, 1, nullptr, R.data()) == TO_OK, "DiagonalQuatCost, one block: %s", g_err.c_str());
  // zero and negative weights pass: to_set_cost asks nothing of a descriptor's Q and R either (definiteness is a warning in the reference)
  Q[5] = 0.0; R[3] = -1.0;
  CHECK(validate_cost_weights(&f, 0, Q.data(), R.data()) == TO_OK, "zero / negative weights are the caller's business: %s", g_err.c_str());
  Q[5] = 1.0; R[3] = 0.5;
  report("null_handle", validate_cost_weights(nullptr, 0, Q.data(), R.data()));
  report("null_handle_get", validate_cost_weights_get(nullptr, 0, Q.data(), R.data()));
  report("null_handle_clear", validate_cost_weights_target("to_clear_cost_weights_batch", nullptr, -1, true));
  report("id_low", validate_cost_weights(&f, -1, Q.data(), R.data()));
  report("id_high", validate_cost_weights(&f, NC, Q.data(), R.data()));
  report("id_high_get", validate_cost_weights_get(&f, NC, Q.data(), R.data()));
  report("both_null", validate_cost_weights(&f, 0, nullptr, nullptr));
  report("both_null_get", validate_cost_weights_get(&f, 0, nullptr, nullptr));
  CostWeightFacts busy = facts(c, 3, true);
  report("in_flight", validate_cost_weights(&busy, 0, Q.data(), R.data()));
  report("in_flight_clear", validate_cost_weights_target("to_clear_cost_weights_batch", &busy, -1, true));
  Q[(size_t)n * 37 + 2] = std::numeric_limits<double>::quiet_NaN();
  Q[(size_t)n * 50 + 1] = std::numeric_limits<double>::infinity();
  report("nan_Q", validate_cost_weights(&f, 0, Q.data(), R.data()));
  Q[(size_t)n * 37 + 2] = 1.0; Q[(size_t)n * 50 + 1] = 1.0;
  R[(size_t)m * 69 + 1] = -std::numeric_limits<double>::infinity();
  report("inf_R", validate_cost_weights(&f, 0, Q.data(), R.data()));
  CHECK(validate_cost_weights(&f, 0, Q.data(), nullptr) == TO_OK, "a block that is not given is not looked at");
  R[(size_t)m * 69 + 1] = 0.5;
  const auto cq = costs(TO_COST_QUADRATIC), ce = costs(TO_COST_ERROR_QUADRATIC);
  CostWeightFacts fq = facts(cq), fe = facts(ce, 4);
  report("quadratic", validate_cost_weights(&fq, 2, Q.data(), R.data()));
  report("error_quadratic", validate_cost_weights(&fe, 2, Q.data(), R.data()));
  report("quadratic_get", validate_cost_weights_get(&fq, 2, Q.data(), R.data()));
  CHECK(validate_cost_weights(&fq, 0, Q.data(), R.data()) == TO_OK, "a diagonal cost next to a dense one is accepted: %s", g_err.c_str());
  for (int key : {7, 8, 9, 11}) {
    CostWeightFacts fm = facts(c, key);
    char name[32];
    snprintf(name, sizeof name, "model_%d", key);
    report(name, validate_cost_weights(&fm, 0, Q.data(), R.data()));
  }
  CostWeightFacts fm = facts(c, 8);
  report("model_8_clear", validate_cost_weights_target("to_clear_cost_weights_batch", &fm, -1, true));
  CostWeightFacts ft = facts(c, 3, false, 60);
  report("tracking_first", validate_cost_weights(&ft, 0, Q.data(), R.data()));
  CHECK(validate_cost_weights_get(&ft, 0, Q.data(), R.data()) == TO_OK, "the getter works next to a tracking reference");
  // the other order: a handle with weights refuses a tracking reference (and a window)
  std::vector<int> index(NC);
  for (int k = 0; k < NC; ++k) index[k] = k;
  std::vector<double> Xref((size_t)n * 5 * B, 0.0);
  TrackFacts tf{3, "Cartpole", n, m, NC, B, c.data(), NC, index.data(), false, 0, 0};
  CHECK(validate_tracking_reference(tf, 5, Xref.data(), nullptr, nullptr, TO_TRACK_END_REFUSE) == TO_OK, "without weights the reference is accepted: %s", g_err.c_str());
  tf.cost_weights = true;
  report("weights_first", validate_tracking_reference(tf, 5, Xref.data(), nullptr, nullptr, TO_TRACK_END_REFUSE));
}

// the host copy: filled with every cost's descriptor values, one cost's rows replaced, one cost restarted; the tiling
static void lowering() {
  auto c = costs();
  const int nz = n + m;
  const size_t L = (size_t)NC * nz;
  std::vector<double> v;
  cost_weights_fill(n, m, B, c.data(), NC, &v);
  CHECK(v.size() == L * B, "host copy holds L * B values");
  for (int b = 0; b < B; ++b)
    for (int ci = 0; ci < NC; ++ci) {
      for (int i = 0; i < n; ++i) CHECK(v[L * b + ci * nz + i] == c[ci].Q[i], "fill Q");
      for (int j = 0; j < m; ++j) CHECK(v[L * b + ci * nz + n + j] == c[ci].R[j], "fill R");
    }
  std::vector<double> Q((size_t)n * B), R((size_t)m * B);
  for (int b = 0; b < B; ++b) { for (int i = 0; i < n; ++i) Q[i + (size_t)n * b] = 1000.0 * b + i; for (int j = 0; j < m; ++j) R[j + (size_t)m * b] = -1000.0 * b - j; }
  cost_weights_store(n, m, B, NC, 1, Q.data(), nullptr, &v);   // R = NULL: that block stays
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < n; ++i) CHECK(v[L * b + 1 * nz + i] == Q[i + (size_t)n * b], "store Q");
    for (int j = 0; j < m; ++j) CHECK(v[L * b + 1 * nz + n + j] == c[1].R[j], "store leaves R");
    for (int i = 0; i < nz; ++i) CHECK(v[L * b + 0 * nz + i] == (i < n ? c[0].Q[i] : c[0].R[i - n]) && v[L * b + 2 * nz + i] == (i < n ? c[2].Q[i] : c[2].R[i - n]), "store leaves the other costs");
  }
  cost_weights_store(n, m, B, NC, 2, nullptr, R.data(), &v);
  std::vector<double> tiled;
  cost_weights_tile(n, m, B, Bp, c.data(), NC, v, &tiled);
  CHECK(tiled.size() == cost_weights_tiled_len(n, m, NC, Bp) && tiled.size() == (size_t)(Bp / 64 + 1) * L * 64, "tiled length: Bp / 64 tiles and one spare");
  for (size_t b = 0; b < (size_t)Bp + 64; ++b)
    for (size_t e = 0; e < L; ++e) {
      const int ci = (int)(e / nz), i = (int)(e % nz);
      const double shared = i < n ? c[ci].Q[i] : c[ci].R[i - n];
      const double want = b < (size_t)B ? v[L * b + e] : shared;   // the lanes behind the batch and the spare tile: the descriptors' values
      CHECK(tiled[((b >> 6) * L + e) * 64 + (b & 63)] == want, "tiled entry %zu of trajectory %zu", e, b);
    }
  CHECK(tiled[((69 >> 6) * L + 2 * nz + n + 1) * 64 + (69 & 63)] == -69001.0, "R_1 of cost 2 of trajectory 69");
  // to_set_cost on cost 1: its rows start over from the new descriptor, the others keep what was set
  c[1].Q[0] = 77.0;
  cost_weights_restart(n, m, B, c.data(), NC, 1, &v);
  for (int b = 0; b < B; ++b) {
    CHECK(v[L * b + nz] == 77.0 && v[L * b + nz + 1] == c[1].Q[1], "restart: cost 1 on its new descriptor");
    CHECK(v[L * b + 2 * nz + n] == R[(size_t)m * b], "restart: cost 2 keeps its weights");
  }
}

// routing: a cost_weights handle plans what a con_limits handle plans, apart from the preloaded stage cost; without the flag everything is as it is today
struct Model { const char* name; int ne, m; PathTraits t; };
static PathTraits traits(bool wt, bool mfma, bool coop, bool lane, int ls, bool eb, bool ebc, bool ebs, bool ar, bool elk, bool ec, uint32_t f, uint32_t f2, uint32_t fp) {
  PathTraits t;
  t.write_through = wt; t.mfma_backward = mfma; t.coop_backward = coop; t.lane_backward = lane; t.ls_first_round = ls;
  t.expand_backward = eb; t.expand_backward_coop = ebc; t.expand_backward_scan = ebs; t.accept_roll = ar; t.expand_lane_k = elk; t.expand_const = ec;
  t.forward = f; t.forward2 = f2; t.forward_plants = fp;
  return t;
}
static const Model MODELS[] = {   // the trait sets of tests/host_shim/constraint_limits_plan_harness.cpp
    {"double integrator 2", 4, 2, traits(true, false, true, true, 4, true, true, true, true, true, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"cartpole", 4, 1, traits(true, true, true, true, 4, true, true, true, true, true, false, 0xFFFFu, 0xFFFFu, 0x5500u)},
    {"quadrotor", 12, 4, traits(false, true, false, false, 16, false, false, false, true, false, true, 0x0F0Fu | (3u << 18) | (3u << 26), 0x0F0Fu | (3u << 18) | (3u << 26), 0x0500u)},
};
static std::string g_envs;
static const char* lookup(const char* name) {
  static std::string val;
  const std::string key = std::string(name).substr(8) + "=";   // without TRAJOPT_
  size_t i = 0;
  while (i < g_envs.size()) {
    const size_t sp = g_envs.find(' ', i) == std::string::npos ? g_envs.size() : g_envs.find(' ', i);
    if (g_envs.compare(i, key.size(), key) == 0) { val = g_envs.substr(i + key.size(), sp - i - key.size()); return val.c_str(); }
    i = sp + 1;
  }
  return nullptr;
}
static bool same_step(const StepPlan& a, const StepPlan& b) { return a.kind == b.kind && a.CW == b.CW && a.TW == b.TW && a.two_wave == b.two_wave && a.store_x == b.store_x && a.two_launch == b.two_launch; }

static void routing(const Model& M, int Bt, int N, bool dense, bool cons, bool non_selector, bool diag, const char* env) {
  g_envs = env;
  PathShape sh;
  sh.B = Bt; sh.Bp = (Bt + 63) / 64 * 64; sh.N = N; sh.ne = M.ne; sh.m = M.m; sh.n_cons = cons ? 2 : 0; sh.diagonal_cost_blocks = diag;
  const PathPlan p = plan_paths(M.t, sh, read_path_knobs(lookup));
  char what[200];
  snprintf(what, sizeof what, "%s B=%d N=%d dense=%d cons=%d generic=%d diag=%d [%s]", M.name, Bt, N, (int)dense, (int)cons, (int)non_selector, (int)diag, env);
  TableFlags base;
  base.dense_costs = dense; base.cons = cons; base.non_selector = cons && non_selector;
  CHECK(!base.cost_weights, "TableFlags::cost_weights defaults to false");
  TableFlags gw = base, cl = base, both = base;
  gw.cost_weights = true; cl.con_limits = true; both.cost_weights = both.con_limits = true;
  const int ev0 = expand_variant_of(base), evw = expand_variant_of(gw), evl = expand_variant_of(cl);
  CHECK(evw == evl && evw == expand_variant_of(both) && (evw & 4) && (evw & 3) == (ev0 & 3), "%s: variants weights %d limits %d unflagged %d", what, evw, evl, ev0);
  TableFlags again = gw; again.cost_weights = false;   // to_clear_cost_weights_batch
  CHECK(expand_variant_of(again) == ev0, "%s: variant after clear", what);
  // without the flag: the variant of every combination of the other flags is what the same flags gave before the field existed
  for (int bits = 0; bits < 16; ++bits) {
    TableFlags f = base;
    f.con_params = bits & 1; f.con_limits = bits & 2; f.plants = bits & 4; f.time_steps = bits & 8;
    const bool generic = f.non_selector || f.con_params || f.con_limits || f.plants || f.time_steps;
    CHECK(expand_variant_of(f) == ((dense ? 1 : 0) | (cons ? 2 : 0) | (generic ? 4 : 0)), "%s: unflagged variant with flags %d", what, bits);
  }
  const int hd = (!p.bwd_mfma && !p.bwd_lane && diag) ? 1 : 0;
  const int counts[] = {0, 1, 63, 64, 65, Bt / 4, Bt / 2, Bt - 1, Bt, p.deep_max_active, p.deep_max_active + 1, p.scan_max_active, 2047, 2048, 32767, 32768};
  for (int la : counts) {
    if (la < 0 || la > Bt) continue;
    for (int armed = 0; armed <= 1; ++armed) {
      const StepPlan sw = plan_step(p, M.t, hd, evw, armed, la, Bt), sl = plan_step(p, M.t, hd, evl, armed, la, Bt), s0 = plan_step(p, M.t, hd, ev0, armed, la, Bt);
      ++flagged; ++plain;
      CHECK(same_step(sw, sl), "%s: %d active: the weights step differs from the limits step", what, la);
      CHECK(sw.kind != STEP_SCAN && sw.kind != STEP_FUSED_COOP, "%s: %d active: step kind %d with per-trajectory weights", what, la, (int)sw.kind);
      CHECK(sw.CW == s0.CW && sw.TW == s0.TW && sw.two_wave == s0.two_wave && sw.store_x == s0.store_x && sw.two_launch == s0.two_launch, "%s: %d active: shape / stores change with the flag", what, la);
      lane_flagged += sw.kind == STEP_FUSED_LANE; two_wave_flagged += sw.two_wave; fused_plain += s0.kind == STEP_FUSED_COOP || s0.kind == STEP_SCAN;
    }
  }
  for (int h : {0, 1}) {
    CHECK(!fused_coop_now(p, h, evw) && !scan_now(p, h, evw), "%s: fused cooperative / scan predicate with the flag", what);
    int32_t a[8], b[8];
    path_report(p, M.t, h, evw, Bt, a); path_report(p, M.t, h, evl, Bt, b);
    CHECK(!std::memcmp(a, b, sizeof a) && a[5] == 0, "%s: report with weights differs from the report with limits", what);
    repack_flagged += (a[7] & 2) != 0;
    // forward-list mode: off with the flag whatever else holds; without it, the trailing argument changes nothing
    for (int al = 0; al <= 1; ++al)
      for (int f2 = 0; f2 <= 1; ++f2) {
        CHECK(!solve_forward_list(p, M.t, h, evw, 0, al, Bt, sh.Bp, false, false, f2, true, 1 << 30, true), "%s: list mode with weights", what);
        CHECK(!solve_forward_list(p, M.t, h, ev0, 0, al, Bt, sh.Bp, false, false, f2, true, 1 << 30, true), "%s: list mode with the flag alone", what);
        CHECK(solve_forward_list(p, M.t, h, ev0, 0, al, Bt, sh.Bp, false, false, f2, true, 1 << 30, false) ==
                  solve_forward_list(p, M.t, h, ev0, 0, al, Bt, sh.Bp, false, false, f2, true, 1 << 30), "%s: list mode without the flag", what);
      }
  }
  for (int simple = 0; simple <= 1; ++simple)
    for (int rk4 = 0; rk4 <= 1; ++rk4)
      for (int unit = 0; unit <= 1; ++unit)
        for (int gl = 0; gl <= 1; ++gl) {
          // flagged: a general variant that does NOT preload the stage cost — the limits handle's variant with bit 0 cleared
          CHECK(forward_general(ev0, gl, false, false, true) && !forward_simple(simple, true), "%s: forward pass with weights", what);
          const int mw = forward_mode(forward_simple(simple, true), cons, rk4, forward_general(evw, gl, false, false, true), unit, M.t.forward);
          const int ml = forward_mode(false, cons, rk4, forward_general(evl, gl, false, true), unit, M.t.forward);
          CHECK(mw == ml && (mw < 0 || ((mw & 8) && !(mw & 1))), "%s: forward variant %d with weights, %d with limits and no simple stage", what, mw, ml);
          // unflagged: the defaulted arguments give today's request, for every combination of the other arrays
          for (int cp = 0; cp <= 1; ++cp)
            for (int clim = 0; clim <= 1; ++clim) {
              const bool was = (ev0 & 5) != 0 || gl || cp || clim;
              CHECK(forward_general(ev0, gl, cp, clim) == was && forward_general(ev0, gl, cp, clim, false) == was && forward_simple(simple) == (simple != 0) &&
                        forward_simple(simple, false) == (simple != 0), "%s: unflagged forward request", what);
              simple_plain += forward_mode(forward_simple(simple), cons, rk4, forward_general(ev0, gl, cp, clim), unit, M.t.forward) & 1;
            }
        }
}

// the repacked working set: a set sized with the weights is told from one sized without, also where another array has their row length
static void repack_rule() {
  const int L = NC * (n + m);
  const std::vector<RpSlot> plain_set = {{0, 41 * 4}, {0, 40}, {0, 4}, {1, 1}, {2, 1}};
  std::vector<RpSlot> with_gl = plain_set, with_gw = plain_set, with_cp = plain_set, with_both = plain_set;
  with_gl.insert(with_gl.begin() + 3, {0, L});
  with_gw.insert(with_gw.begin() + 3, {4, L});
  with_cp.insert(with_cp.begin() + 3, {3, L});     // per-trajectory constraint parameters that happen to have the same row length
  with_both.insert(with_both.begin() + 3, {0, L}); with_both.insert(with_both.begin() + 4, {4, L});
  RpSized have;
  have.slots = with_gw; have.cap = 128;
  CHECK(rp_reusable(have, with_gw, 128) && rp_reusable(have, with_gw, 64), "a set sized with the weights serves the same table again");
  CHECK(!rp_reusable(have, with_gw, 192), "capacity");
  CHECK(!rp_reusable(have, plain_set, 64) && !rp_reusable(have, with_gl, 64) && !rp_reusable(have, with_cp, 64) && !rp_reusable(have, with_both, 64), "a set sized with the weights serves no other table");
  for (const std::vector<RpSlot>* other : {(const std::vector<RpSlot>*)&plain_set, (const std::vector<RpSlot>*)&with_gl, (const std::vector<RpSlot>*)&with_cp, (const std::vector<RpSlot>*)&with_both}) {
    RpSized h2;
    h2.slots = *other; h2.cap = 128;
    CHECK(rp_reusable(h2, *other, 64) && (other == &with_both || !rp_reusable(h2, with_gw, 64)), "a set sized without the weights does not serve a table with them");
  }
  CHECK(rp_slot_bytes({4, L}, 128) == sizeof(double) * L * 128 && rp_slot_bytes({4, L}, 128) == rp_slot_bytes({3, L}, 128), "the weights are a tiled array of doubles");
  CHECK(rp_device_kind(4) == 3 && rp_device_kind(3) == 3 && rp_device_kind(0) == 0 && rp_device_kind(1) == 1 && rp_device_kind(2) == 2, "the kernels move the weights like cp / cl: never copied home");
  CHECK(rp_tiled(0) && rp_tiled(3) && rp_tiled(4) && !rp_tiled(1) && !rp_tiled(2), "tiled kinds");
}

int main() {
  refusals();
  lowering();
  const char* envs[] = {"", "BACKWARD=lane", "BACKWARD=lane ACCEPT_ROLL_MIN=1", "BACKWARD=coop", "BACKWARD=mfma", "SCAN=2", "FUSED_LANE=0", "FWD2=1", "REPACK=64 BACKWARD=lane", "COMPACT=0"};
  for (const Model& M : MODELS)
    for (int Bt : {1, 24, 40, 70, 300, 1024, 12288, 70000})
      for (int N : {31, 41, 101})
        for (int dense = 0; dense <= 1; ++dense)
          for (int cons = 0; cons <= 1; ++cons)
            for (int generic = 0; generic <= 1; ++generic)
              for (int diag = 0; diag <= 1; ++diag)
                for (const char* env : envs) routing(M, Bt, N, dense != 0, cons != 0, generic != 0, diag != 0, env);
  repack_rule();
  printf("flagged %lld plain %lld lane_flagged %lld two_wave_flagged %lld repack_flagged %lld fused_plain %lld simple_plain %lld\n", flagged, plain, lane_flagged, two_wave_flagged,
         repack_flagged, fused_plain, simple_plain);
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
