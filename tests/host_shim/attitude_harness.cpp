// Compiles the host-only side of per-trajectory attitude references as a program of its own (test infrastructure; tests/test_cost_attitude_host.py,
// which builds it with -fsanitize=address,undefined as well): csrc/desc_lower.h — every refusal of to_set_cost_attitude_batch / to_get_... /
// to_clear_... / to_set_tracking_attitude, the image of DevProblem::ga and its tiling —, csrc/path_plan.h — the rules by which ga rides on gw
// (cost_lane_step) and the routing that results — and csrc/k_track.h, the kernel of the tracking lowering, run thread by thread with every
// array at exactly the size the entry points give it.  Prints
//   case <name> code <c> msg <text>     every refusal, with the error class and the message;
//   state <sequence> ...                the state machine after every step of every sequence;
//   "checks <n> fails <n>".
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; };
static dim3 blockIdx, threadIdx, gridDim;
#define __launch_bounds__(x)

#include "k_track.h"
#include "desc_lower.h"
#include "path_plan.h"

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

static long long fails = 0, checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static const int n = 13, m = 4, B = 70, Bp = 128, NC = 3;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double next_value() {  // a finite double with a full mantissa, now and then a signed zero (tests/host_shim/track_lower_harness.cpp)
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  if ((g_rng & 63) == 0) return (g_rng & 64) ? -0.0 : 0.0;
  uint64_t bits = (g_rng & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 8 + (g_rng >> 52) % 16) << 52);
  double v;
  std::memcpy(&v, &bits, sizeof v);
  return v;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static std::vector<to_cost_desc> costs(int kind0 = TO_COST_DIAGONAL) {   // cost 1 and 2: DiagonalQuatCost; cost 0: kind0
  std::vector<to_cost_desc> c(NC);
  for (int ci = 0; ci < NC; ++ci) {
    std::memset(&c[ci], 0, sizeof(to_cost_desc));
    c[ci].kind = ci == 0 ? kind0 : TO_COST_DIAGONAL_QUAT;
    for (int i = 0; i < n; ++i) c[ci].Q[i] = 10.0 * (ci + 1) + i;
    for (int j = 0; j < m; ++j) c[ci].R[j] = 0.1 * (ci + 1) + 0.01 * j;
    for (int i = 0; i < 4; ++i) { c[ci].q_ref[i] = 0.25 * (ci + 1) + 0.01 * i; c[ci].q_ind[i] = 4 + i; }
  }
  return c;
}
static const char* NAMES[] = {"double integrator (D = 1)", "double integrator (D = 2)", "double integrator (D = 3)", "Cartpole", "Quadrotor", "Quadrotor{MRP}",
                              "Quadrotor{RodriguesParam}", "hybrid double integrator", "model vector", "InfeasibleModel (double integrator, D = 1)",
                              "InfeasibleModel (double integrator, D = 2)", "InfeasibleModel (Cartpole)"};
static CostWeightFacts facts(const std::vector<to_cost_desc>& c, int key = 4, bool in_flight = false, int Nref = 0) {
  return CostWeightFacts{key, NAMES[key], n, m, B, c.data(), (int)c.size(), in_flight, Nref};
}
static void report(const char* name, int rc) { printf("case %s code %d msg %s\n", name, rc, g_err.c_str()); g_err.clear(); }

static void refusals() {
  const auto c = costs();
  std::vector<double> A((size_t)4 * B, 0.5);
  CostWeightFacts f = facts(c);
  CHECK(validate_cost_attitude(&f, 1, A.data()) == TO_OK && validate_cost_attitude(&f, 2, A.data()) == TO_OK, "a plain call is accepted: %s", g_err.c_str());
  // used as given: not normalised, any sign, zero
  A[5] = -3.0; A[6] = 0.0;
  CHECK(validate_cost_attitude(&f, 1, A.data()) == TO_OK, "the values are the caller's business: %s", g_err.c_str());
  A[5] = A[6] = 0.5;
  report("null_handle", validate_cost_attitude(nullptr, 1, A.data()));
  report("null_handle_get", validate_cost_attitude_get(nullptr, 1, A.data()));
  report("null_handle_clear", validate_cost_weights_target("to_clear_cost_attitude_batch", nullptr, -1, true));
  report("null_handle_track", validate_tracking_attitude(nullptr, 1));
  report("null_q_ref", validate_cost_attitude(&f, 1, nullptr));
  report("null_q_ref_get", validate_cost_attitude_get(&f, 1, nullptr));
  report("id_low", validate_cost_attitude(&f, -1, A.data()));
  report("id_high", validate_cost_attitude(&f, NC, A.data()));
  report("id_high_get", validate_cost_attitude_get(&f, NC, A.data()));
  CostWeightFacts busy = facts(c, 4, true);
  report("in_flight", validate_cost_attitude(&busy, 1, A.data()));
  report("in_flight_get", validate_cost_attitude_get(&busy, 1, A.data()));
  report("in_flight_clear", validate_cost_weights_target("to_clear_cost_attitude_batch", &busy, -1, true));
  A[(size_t)4 * 37 + 2] = std::numeric_limits<double>::quiet_NaN();
  A[(size_t)4 * 50 + 1] = std::numeric_limits<double>::infinity();
  report("nan", validate_cost_attitude(&f, 1, A.data()));
  A[(size_t)4 * 37 + 2] = 0.5;
  report("inf", validate_cost_attitude(&f, 1, A.data()));
  A[(size_t)4 * 50 + 1] = 0.5;
  report("diagonal", validate_cost_attitude(&f, 0, A.data()));
  report("diagonal_get", validate_cost_attitude_get(&f, 0, A.data()));
  const auto cq = costs(TO_COST_QUADRATIC), ce = costs(TO_COST_ERROR_QUADRATIC);
  CostWeightFacts fq = facts(cq), fe = facts(ce);
  report("quadratic", validate_cost_attitude(&fq, 0, A.data()));
  report("error_quadratic", validate_cost_attitude(&fe, 0, A.data()));
  CHECK(validate_cost_attitude(&fe, 1, A.data()) == TO_OK, "a DiagonalQuatCost next to an ErrorQuadratic is accepted: %s", g_err.c_str());
  for (int key : {7, 8, 9, 11}) {
    CostWeightFacts fm = facts(c, key);
    char name[32];
    snprintf(name, sizeof name, "model_%d", key);
    report(name, validate_cost_attitude(&fm, 1, A.data()));
  }
  CostWeightFacts fm = facts(c, 8);
  report("model_8_clear", validate_cost_weights_target("to_clear_cost_attitude_batch", &fm, -1, true));
  // next to a stored tracking reference the setter is accepted (the weights setter is not)
  CostWeightFacts ft = facts(c, 4, false, 60);
  CHECK(validate_cost_attitude(&ft, 1, A.data()) == TO_OK, "accepted next to a tracking reference: %s", g_err.c_str());
  std::vector<double> Q((size_t)n * B, 1.0);
  CHECK(validate_cost_weights(&ft, 1, Q.data(), nullptr) == TO_ERR_UNSUPPORTED, "the weights setter still refuses a handle with a tracking reference");
  // to_set_tracking_attitude
  std::vector<int> index(NC);
  for (int k = 0; k < NC; ++k) index[k] = k;
  TrackFacts tf{4, "Quadrotor", n, m, NC, B, c.data(), NC, index.data(), false, 0, 0};
  report("track_no_reference", validate_tracking_attitude(&tf, 1));
  CHECK(validate_tracking_attitude(&tf, 0) == TO_OK, "off needs nothing: %s", g_err.c_str());
  tf.Nref_set = 30;
  CHECK(validate_tracking_attitude(&tf, 1) == TO_OK, "on with a reference and a DiagonalQuatCost: %s", g_err.c_str());
  report("track_bad_flag", validate_tracking_attitude(&tf, 2));
  TrackFacts tb = tf; tb.in_flight = true;
  report("track_in_flight", validate_tracking_attitude(&tb, 1));
  std::vector<to_cost_desc> plain = c;
  for (auto& d : plain) d.kind = TO_COST_DIAGONAL;
  TrackFacts tp = tf; tp.costs = plain.data();
  report("track_no_quat", validate_tracking_attitude(&tp, 1));
}

// the image of ga: every cost's descriptor values, the tiling with its spare tile, one cost's rows
static void lowering() {
  const auto c = costs();
  const size_t L = (size_t)4 * NC;
  std::vector<double> v, tiled, rows;
  cost_attitude_fill(B, c.data(), NC, &v);
  CHECK(v.size() == L * B, "host image holds L * B values");
  for (int b = 0; b < B; ++b)
    for (int ci = 0; ci < NC; ++ci)
      for (int i = 0; i < 4; ++i) CHECK(v[L * b + 4 * ci + i] == c[ci].q_ref[i], "fill");
  for (int b = 0; b < B; ++b) for (int i = 0; i < 4; ++i) v[L * b + 4 * 1 + i] = 1000.0 * b + i;   // what the setter's rows look like for cost 1
  cost_attitude_tile(B, Bp, c.data(), NC, v, &tiled);
  CHECK(tiled.size() == cost_attitude_tiled_len(NC, Bp) && tiled.size() == (size_t)(Bp / 64 + 1) * L * 64, "tiled length: Bp / 64 tiles and one spare");
  for (size_t b = 0; b < (size_t)Bp + 64; ++b)
    for (size_t e = 0; e < L; ++e) {
      const double want = b < (size_t)B ? v[L * b + e] : c[e / 4].q_ref[e % 4];   // the lanes behind the batch and the spare tile: the descriptors' values
      CHECK(tiled[((b >> 6) * L + e) * 64 + (b & 63)] == want, "tiled entry %zu of trajectory %zu", e, b);
    }
  CHECK(tiled[((69 >> 6) * L + 4 * 1 + 3) * 64 + (69 & 63)] == 69003.0, "q_ref[3] of cost 1 of trajectory 69");
  cost_attitude_rows(B, c[2], &rows);
  CHECK(rows.size() == (size_t)4 * B, "one cost's rows");
  for (int b = 0; b < B; ++b) for (int i = 0; i < 4; ++i) CHECK(rows[i + 4 * b] == c[2].q_ref[i], "restart rows");
}

// ---- the state machine: what gw holds, which routing results, which refusals fire ----------------------------------------------------------
// cost_lane_step (path_plan.h) is the library's own code.  Model is NOT: it restates, in a dozen lines, what trajopt_hip.hip cost_lane_apply and
// the entry points do with the actions (fill from the descriptors, store the caller's values, release); gw / ga say what the arrays then hold.
// What the library really leaves in the device arrays is checked on the GPU (tests/test_gpu_cost_attitude.py::test_setter_semantics).
enum Holds { NONE, DESCRIPTORS, CALLER };
struct Model {
  CostLaneState s;
  Holds gw = NONE, ga = NONE;
  void apply(CostLaneEvent e) {
    const CostLaneAction a = cost_lane_step(&s, e);
    if (a.release || !s.routed()) { gw = ga = NONE; CHECK(!s.routed(), "released while a reason stands"); return; }
    if (a.fill_gw) gw = DESCRIPTORS;
    if (a.fill_ga) ga = DESCRIPTORS;
    if (e == LANE_SET_WEIGHTS) gw = CALLER;
    if (e == LANE_SET_ATTITUDE || e == LANE_TRACK_ON) ga = CALLER;
    if (e == LANE_TRACK_OFF && !s.attitude) ga = DESCRIPTORS;   // (tracking_attitude_off restarts the rows itself)
  }
};
static void check_state(const Model& M, const char* seq, int step) {
  const bool routed = M.s.routed();
  // both arrays stand or neither does; gw holds the caller's values exactly while the caller's flag is up
  CHECK((M.gw != NONE) == routed && (M.ga != NONE) == routed, "%s step %d: arrays vs routing", seq, step);
  CHECK((M.gw == CALLER) == M.s.weights, "%s step %d: gw holds %d with weights = %d", seq, step, (int)M.gw, (int)M.s.weights);
  CHECK(!routed || M.s.attitude || M.s.track_attitude || M.ga == DESCRIPTORS, "%s step %d: ga without attitudes must hold the descriptors", seq, step);
  // routing: TableFlags::cost_weights follows the arrays, and with it the variant and the forward request of a weights handle
  TableFlags f;
  f.cost_weights = routed;
  CHECK(((expand_variant_of(f) & 4) != 0) == routed && forward_general(0, false, false, false, routed) == routed && forward_simple(true, routed) == !routed,
        "%s step %d: routing", seq, step);
  // refusals: the tracking calls look at the caller's weights alone; the weights setter at a stored reference alone
  const auto c = costs();
  std::vector<int> index(NC);
  for (int k = 0; k < NC; ++k) index[k] = k;
  std::vector<double> X((size_t)n * 5 * B, 0.0);
  TrackFacts tf{4, "Quadrotor", n, m, NC, B, c.data(), NC, index.data(), false, 0, 0, M.s.weights};
  const int rc = validate_tracking_reference(tf, 5, X.data(), nullptr, nullptr, TO_TRACK_END_HOLD);
  CHECK(rc == (M.s.weights ? TO_ERR_UNSUPPORTED : TO_OK), "%s step %d: tracking reference -> %d (%s)", seq, step, rc, g_err.c_str());
  tf.Nref_set = 5; tf.end_mode_set = TO_TRACK_END_HOLD;
  std::vector<int32_t> start(B, 1);
  const int rw = validate_tracking_window(tf, start.data());
  CHECK(rw == (M.s.weights ? TO_ERR_UNSUPPORTED : TO_OK), "%s step %d: tracking window -> %d", seq, step, rw);
  printf("state %s step %d weights %d attitude %d track %d routed %d gw %d ga %d\n", seq, step, (int)M.s.weights, (int)M.s.attitude, (int)M.s.track_attitude, (int)routed,
         (int)M.gw, (int)M.ga);
}
static void sequence(const char* name, std::initializer_list<CostLaneEvent> evs) {
  Model M;
  int step = 0;
  check_state(M, name, step);
  for (CostLaneEvent e : evs) { M.apply(e); check_state(M, name, ++step); }
  CHECK(!M.s.routed() && M.gw == NONE && M.ga == NONE, "%s: the sequence ends on a fresh handle's routing", name);
}
static void state_machine() {
  sequence("attitude_only", {LANE_SET_ATTITUDE, LANE_SET_ATTITUDE, LANE_CLEAR_ATTITUDE});
  sequence("attitude_then_weights", {LANE_SET_ATTITUDE, LANE_SET_WEIGHTS, LANE_CLEAR_WEIGHTS, LANE_CLEAR_ATTITUDE});
  sequence("weights_then_attitude", {LANE_SET_WEIGHTS, LANE_SET_ATTITUDE, LANE_CLEAR_ATTITUDE, LANE_CLEAR_WEIGHTS});
  sequence("interleaved", {LANE_SET_WEIGHTS, LANE_SET_ATTITUDE, LANE_CLEAR_WEIGHTS, LANE_SET_WEIGHTS, LANE_CLEAR_ATTITUDE, LANE_CLEAR_WEIGHTS});
  sequence("weights_only", {LANE_SET_WEIGHTS, LANE_CLEAR_WEIGHTS, LANE_CLEAR_WEIGHTS});
  sequence("clears_on_a_fresh_handle", {LANE_CLEAR_ATTITUDE, LANE_CLEAR_WEIGHTS, LANE_TRACK_OFF});
  sequence("tracking", {LANE_TRACK_ON, LANE_TRACK_OFF});
  sequence("tracking_and_setter", {LANE_TRACK_ON, LANE_SET_ATTITUDE, LANE_TRACK_OFF, LANE_CLEAR_ATTITUDE});
  sequence("tracking_then_clear", {LANE_TRACK_ON, LANE_CLEAR_ATTITUDE, LANE_TRACK_OFF});
  // single steps: what each asks of the arrays
  CostLaneState s;
  CostLaneAction a = cost_lane_step(&s, LANE_SET_ATTITUDE);
  CHECK(a.fill_gw && a.fill_ga && !a.release, "first use fills both arrays from the descriptors");
  a = cost_lane_step(&s, LANE_SET_WEIGHTS);
  CHECK(!a.fill_gw && !a.fill_ga && !a.release, "weights onto an attitude handle: the arrays stand");
  a = cost_lane_step(&s, LANE_CLEAR_WEIGHTS);
  CHECK(a.fill_gw && !a.fill_ga && !a.release && s.routed(), "to_clear_cost_weights_batch next to attitudes: gw back on the descriptors, routing kept");
  a = cost_lane_step(&s, LANE_CLEAR_WEIGHTS);
  CHECK(!a.fill_gw && !a.fill_ga && !a.release, "a second clear does nothing");
  a = cost_lane_step(&s, LANE_CLEAR_ATTITUDE);
  CHECK(a.release && !s.routed(), "the last reason gone: released");
  // to_set_cost in between: one cost's rows restart in both arrays, the state does not move (the library calls cost_weights_restart / cost_attitude_rows)
  auto c = costs();
  std::vector<double> gw;
  cost_weights_fill(n, m, B, c.data(), NC, &gw);
  c[1].Q[0] = 77.0; c[1].q_ref[2] = -0.5;
  cost_weights_restart(n, m, B, c.data(), NC, 1, &gw);
  std::vector<double> rows;
  cost_attitude_rows(B, c[1], &rows);
  CHECK(gw[(size_t)NC * (n + m) * 5 + (n + m)] == 77.0 && rows[2 + 4 * 5] == -0.5 && rows[1 + 4 * 69] == c[1].q_ref[1], "to_set_cost restarts that cost's rows from the new descriptor");
}

// ---- k_track_lower with attitude rows ------------------------------------------------------------------------------------------------------
static void run(const TrackArgs& a, unsigned gx, unsigned gy) {
  gridDim.x = gx; gridDim.y = gy;
  for (blockIdx.y = 0; blockIdx.y < gy; ++blockIdx.y)
    for (blockIdx.x = 0; blockIdx.x < gx; ++blockIdx.x)
      for (threadIdx.x = 0; threadIdx.x < 64; ++threadIdx.x) k_track_lower(a);
}
static std::unique_ptr<double[]> filled(size_t count) {
  std::unique_ptr<double[]> p(new double[count]);
  for (size_t i = 0; i < count; ++i) p[i] = next_value();
  return p;
}
static const int ODD_IND[4] = {7, 4, 13, 1};   // a q_ind that is not the default 4:7
static void track_case(int N, int Bt, int Nref, int start_mode, bool with_u, bool attitude, bool wide, bool odd_ind) {
  const int nz = n + m, tiles = (Bt + 63) / 64, n_costs = N + 1, Lr = Nref * nz, L = n_costs * nz, La = n_costs * 4;
  std::unique_ptr<to_cost_desc[]> cs(new to_cost_desc[n_costs]);
  for (int c = 0; c < n_costs; ++c) {
    std::memset(&cs[c], 0, sizeof(to_cost_desc));
    cs[c].kind = c % 3 == 2 ? TO_COST_DIAGONAL : TO_COST_DIAGONAL_QUAT;   // a third of the knots carry a cost of another kind
    for (int i = 0; i < TO_MAX_N; ++i) { cs[c].Q[i] = next_value(); cs[c].q[i] = next_value(); }
    for (int i = 0; i < TO_MAX_M; ++i) { cs[c].R[i] = next_value(); cs[c].r[i] = next_value(); }
    for (int i = 0; i < 4; ++i) { cs[c].q_ref[i] = next_value(); cs[c].q_ind[i] = odd_ind ? ODD_IND[i] : 4 + i; }
  }
  std::unique_ptr<int[]> cost_index(new int[N]);
  for (int k = 0; k < N; ++k) cost_index[k] = (k * 3 + 1) % n_costs;
  std::unique_ptr<int[]> start(new int[Bt]);
  for (int b = 0; b < Bt; ++b) start[b] = start_mode == 0 ? 1 : start_mode == 1 ? 1 + b % (Nref - N + 1 > 1 ? Nref - N + 1 : 3) : 1 + (b * 5 + 2) % Nref;   // mode 2: past the end
  auto ref = filled((size_t)tiles * Lr * 64), gl = filled((size_t)tiles * L * 64), ga = filled((size_t)tiles * La * 64);   // (ga: no spare tile needed here — the kernel stays inside the batch's tiles)
  std::vector<double> ga_old(ga.get(), ga.get() + (size_t)tiles * La * 64);
  TrackArgs a;
  std::memset(&a, 0, sizeof a);
  a.n = n; a.m = m; a.N = N; a.B = Bt; a.Nref = Nref; a.with_u = with_u ? 1 : 0; a.n_costs = n_costs;
  a.ref = ref.get(); a.start = start.get(); a.cost_index = cost_index.get(); a.costs = cs.get(); a.gl = gl.get(); a.ga = attitude ? ga.get() : nullptr;
  const int rows = N * (with_u ? nz : n) + (attitude ? 4 * N : 0);
  run(a, (unsigned)tiles, (unsigned)(wide ? (rows < 32 ? rows : 32) : 1));
  auto tiled = [](const double* p, int Ld, int b, int e) { return p[((size_t)(b >> 6) * Ld + e) * 64 + (b & 63)]; };
  std::vector<int> knot_of(n_costs, -1);
  for (int k = 0; k < N; ++k) knot_of[cost_index[k]] = k;
  for (int b = 0; b < tiles * 64; ++b)
    for (int c = 0; c < n_costs; ++c) {
      const int k = knot_of[c];
      const bool written = attitude && b < Bt && k >= 0 && cs[c].kind == TO_COST_DIAGONAL_QUAT;
      int j = k >= 0 && b < Bt ? start[b] - 1 + k : 0;
      if (j > Nref - 1) j = Nref - 1;
      for (int i = 0; i < 4; ++i) {
        const double want = written ? tiled(ref.get(), Lr, b, j * nz + cs[c].q_ind[i] - 1) : tiled(ga_old.data(), La, b, c * 4 + i);   // an exact copy, or untouched
        CHECK(same_bits(tiled(ga.get(), La, b, c * 4 + i), want), "attitude row %d of cost %d, trajectory %d (N %d B %d Nref %d starts %d att %d)", i, c, b, N, Bt, Nref, start_mode, (int)attitude);
      }
      if (b >= Bt || k < 0) continue;
      // the linear rows: bit for bit the documented recipe, in both modes
      for (int i = 0; i < (with_u ? nz : n); ++i) {
        const bool state = i < n;
        const int r = state ? i : i - n;
        const double z = tiled(ref.get(), Lr, b, j * nz + i);
        const double acc = (state ? cs[c].Q[r] : cs[c].R[r]) * z;
        const double want = (-acc) - (state ? cs[c].q[r] : cs[c].r[r]);
        CHECK(same_bits(tiled(gl.get(), L, b, c * nz + i), want), "linear row %d of cost %d, trajectory %d", i, c, b);
      }
    }
}

int main() {
  refusals();
  lowering();
  state_machine();
  for (int N : {4, 21})   // (n_costs = N + 1 coprime to 3: cost_index is injective)
    for (int Bt : {1, 64, 70, 130})
      for (int Nref : {N, N + 9})
        for (int start_mode = 0; start_mode < 3; ++start_mode)
          for (int with_u = 0; with_u < 2; ++with_u)
            for (int attitude = 0; attitude < 2; ++attitude)
              for (int wide = 0; wide < 2; ++wide) track_case(N, Bt, Nref, start_mode, with_u != 0, attitude != 0, wide != 0, (N + Bt + start_mode) % 2 != 0);
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
