// Compiles the host-only lowering of the oldest entry points (csrc/desc_lower.h: lower_problem — what to_create runs before it asks for a
// device —, lower_constraint_params, cost_linear_delta / cost_linear_zero, plant_params_compatible / validate_plant_params) as a program of its
// own (test infrastructure; tests/test_problem_lower_host.py, which also builds it with -fsanitize=address,undefined).  Prints
//   case <name> code <c> msg <text> : every refusal, with the error class and the message,
// checks the tables lower_problem returns, holds lower_constraint_params bit for bit to the loop it replaced — kept verbatim below, as
// reference_constraint_params — and to its defining property  A shift[inds] = params_b - b0  (zero off inds) with the residual of that loop
// as the tolerance, the linear-term differences exactly, and the plant-parameter rule over every model key and entry.  Ends with
//   max_residual <r>   and   fails <n>.
#include "desc_lower.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)
static void report(const char* name, int rc) { printf("case %s code %d msg %s\n", name, rc, rc == TO_OK ? "" : g_err.c_str()); }

static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double next_value() {  // in (-2, 2), never 0
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return ((double)(g_rng >> 11) + 0.5) * (4.0 / 9007199254740992.0) - 2.0;
}

// ---- A. lower_problem -------------------------------------------------------------------------------------------------------------------
struct Problem {  // a Cartpole problem (n = 4, m = 1) that passes, with the arrays the descriptor points to
  to_problem_desc d;
  std::vector<to_cost_desc> costs;
  std::vector<to_constraint_desc> cons;
  std::vector<double> dt;
  std::vector<int32_t> cost_index;
  std::vector<to_step_model> steps;
  explicit Problem(int N = 5) : costs(2) {
    std::memset(&d, 0, sizeof(d));
    std::memset(costs.data(), 0, sizeof(to_cost_desc) * 2);
    for (auto& c : costs) { c.kind = TO_COST_DIAGONAL; for (int i = 0; i < 4; ++i) c.Q[i] = 1.0; c.R[0] = 0.1; }
    d.abi_version = TO_ABI_VERSION; d.model = TO_MODEL_CARTPOLE; d.integrator = TO_RK4; d.n = 4; d.m = 1; d.N = N; d.B = 3;
    d.model_params[0] = 1.0; d.model_params[1] = 0.2; d.model_params[2] = 0.5; d.model_params[3] = 9.81;
    d.t0 = 0.0; d.tf = 1.0; d.n_costs = 2; d.costs = costs.data();
  }
};
static to_constraint_desc bound_u(int k1, int k2, double lim) {  // finite bounds on the control only: p = 2
  to_constraint_desc c;
  std::memset(&c, 0, sizeof(c));
  c.kind = TO_CON_BOUND; c.sense = TO_CONE_NEGATIVE_ORTHANT; c.k_first = k1; c.k_last = k2; c.n_params = 10;
  for (int i = 0; i < 5; ++i) { c.params[i] = Inf; c.params[5 + i] = -Inf; }
  c.params[4] = lim; c.params[9] = -lim;
  return c;
}
static to_constraint_desc norm_u(int k1, int k2) {  // |u|^2 <= 4: p = 1
  to_constraint_desc c;
  std::memset(&c, 0, sizeof(c));
  c.kind = TO_CON_NORM; c.sense = TO_CONE_NEGATIVE_ORTHANT; c.k_first = k1; c.k_last = k2; c.n_inds = 1; c.inds[0] = 5; c.n_params = 1; c.params[0] = 2.0;
  return c;
}
static to_constraint_desc goal_x(int k, std::vector<int> inds) {
  to_constraint_desc c;
  std::memset(&c, 0, sizeof(c));
  c.kind = TO_CON_GOAL; c.sense = TO_CONE_ZERO; c.k_first = c.k_last = k; c.n_inds = c.n_params = (int)inds.size();
  for (size_t i = 0; i < inds.size(); ++i) { c.inds[i] = inds[i]; c.params[i] = 0.25 * (double)(i + 1); }
  return c;
}
static int lower(const char* name, const to_problem_desc* d, const to_solver_opts* o = nullptr, LoweredProblem* keep = nullptr) {
  LoweredProblem lp;
  lp.n = -7; lp.dt.assign(2, 7.0);
  g_err.clear();
  const int rc = lower_problem(d, o, &lp);
  if (rc != TO_OK) CHECK(lp.n == -7 && lp.dt.size() == 2 && lp.dt[0] == 7.0 && lp.cons.empty() && lp.cost_index.empty(), "%s: the output was touched by a refused call", name);
  report(name, rc);
  if (keep) *keep = lp;
  return rc;
}
static void problem_cases() {
  to_solver_opts good, bad;
  default_opts(&good);
  bad = good; bad.cost_tolerance = -1.0;
  lower("null_desc", nullptr);
  { Problem p; p.d.abi_version = TO_ABI_VERSION + 1; lower("abi", &p.d); }
  { Problem p; lower("opts", &p.d, &bad); }
  { Problem p; p.d.abi_version = 0; lower("order_abi_before_opts", &p.d, &bad); }
  { Problem p; p.d.model = 99; lower("unknown_model", &p.d); }
  { Problem p; p.d.n = 5; lower("dims", &p.d); }
  { Problem p; p.d.N = 1; lower("few_knots", &p.d); }
  { Problem p; p.d.B = 0; lower("batch", &p.d); }
  { Problem p; p.d.tf = p.d.t0; lower("time_span", &p.d); }
  { Problem p; p.d.tf = NaN; lower("time_span_nan", &p.d); }
  { Problem p; p.d.integrator = TO_EULER + 1; lower("integrator", &p.d); }
  { Problem p; p.dt = {0.25, 0.25, 0.0, 0.5}; p.d.dt = p.dt.data(); lower("dt_sign", &p.d); }
  { Problem p; p.dt = {0.25, 0.25, 0.25, 0.5}; p.d.dt = p.dt.data(); lower("dt_sum", &p.d); }
  { Problem p; p.d.n_costs = 0; lower("no_costs", &p.d); }
  { Problem p; p.d.costs = nullptr; lower("null_costs", &p.d); }
  { Problem p; p.costs[1].kind = 17; lower("cost_kind", &p.d); }
  { Problem p(6); p.d.model = TO_MODEL_HYBRID_DOUBLE_INTEGRATOR; p.d.n = 4; p.d.m = 2; p.d.model_params[1] = 5.0; lower("hybrid_steps", &p.d); }
  { Problem p(6); p.d.model = TO_MODEL_HYBRID_DOUBLE_INTEGRATOR; p.d.n = 4; p.d.m = 2; p.d.model_params[1] = 2.5; lower("hybrid_fraction", &p.d); }
  { Problem p; p.d.model = TO_MODEL_VECTOR; p.d.n = TO_VECTOR_N; p.d.m = TO_VECTOR_M; lower("step_models", &p.d); }
  { Problem p; p.cost_index = {0, 1, 2, 0, 1}; p.d.cost_index = p.cost_index.data(); lower("cost_index", &p.d); }
  { Problem p; p.d.n_costs = 1; lower("one_cost", &p.d); }
  { Problem p; p.d.N = 1; p.cost_index = {5}; p.d.cost_index = p.cost_index.data(); lower("order_knots_before_cost_index", &p.d); }
  { Problem p; p.d.n_constraints = -1; lower("con_count", &p.d); }
  { Problem p; p.d.n_constraints = 2; lower("con_null", &p.d); }
  { Problem p; p.cons = {bound_u(1, 4, 3.0), bound_u(1, 4, 3.0)}; p.cons[1].kind = 99; p.d.n_constraints = 2; p.d.constraints = p.cons.data(); lower("con_kind", &p.d); }
  { Problem p; p.cons = {bound_u(1, 6, 3.0)}; p.d.n_constraints = 1; p.d.constraints = p.cons.data(); lower("con_knots", &p.d); }

  // the tables: default steps, given steps at the edge of the tolerance, the default cost_index, dual offsets
  for (int N : {2, 5}) {
    Problem p(N);
    p.d.t0 = 0.3; p.d.tf = 1.7;
    LoweredProblem lp;
    CHECK(lower(N == 2 ? "fine_two_knots" : "fine_five_knots", &p.d, &good, &lp) == TO_OK, "N %d", N);
    CHECK(lp.n == 4 && lp.m == 1 && lp.ne == 4 && lp.key == 3, "N %d: dims %d %d %d key %d", N, lp.n, lp.m, lp.ne, lp.key);
    CHECK((int)lp.dt.size() == N - 1 && lp.step_table.empty() && lp.cons.empty() && lp.n_duals == 0, "N %d: sizes", N);
    for (double v : lp.dt) CHECK(v == (p.d.tf - p.d.t0) / (N - 1), "N %d: default step %.17g", N, v);
    CHECK((int)lp.cost_index.size() == N, "N %d: cost_index", N);
    for (int k = 0; k < N; ++k) CHECK(lp.cost_index[k] == (k == N - 1 ? 1 : 0), "N %d: cost_index[%d] = %d", N, k, lp.cost_index[k]);
  }
  for (int outside = 0; outside < 2; ++outside) {  // |sum - (tf - t0)| against 1e-8 max(1, tf - t0) = 1e-8
    Problem p;
    p.dt = {0.25, 0.25, 0.25, 0.25 + (outside ? 1.01e-8 : 0.99e-8)};
    p.d.dt = p.dt.data();
    LoweredProblem lp;
    const int rc = lower(outside ? "dt_just_outside" : "dt_just_inside", &p.d, nullptr, &lp);
    CHECK(outside ? rc == TO_ERR_ASSERTION : (rc == TO_OK && lp.dt == p.dt), "dt at the tolerance (%d): rc %d", outside, rc);
  }
  {
    Problem p;
    p.cost_index = {1, 0, 0, 1, 0};
    p.d.cost_index = p.cost_index.data();
    p.cons = {bound_u(1, 4, 3.0), norm_u(2, 4), goal_x(5, {1, 2, 3, 4})};  // p = 2 on 4 knots, p = 1 on 3 knots, p = 4 on the terminal knot alone
    p.d.n_constraints = 3; p.d.constraints = p.cons.data();
    LoweredProblem lp;
    CHECK(lower("fine_constrained", &p.d, nullptr, &lp) == TO_OK, "constrained");
    CHECK(lp.cost_index == std::vector<int>({1, 0, 0, 1, 0}), "given cost_index");
    CHECK(lp.cons.size() == 3 && lp.n_duals == 2 * 4 + 1 * 3 + 4 * 1, "n_duals %lld", lp.n_duals);
    if (lp.cons.size() == 3) {
      const long long want_off[3] = {0, 8, 11};
      const int want_p[3] = {2, 1, 4}, want_k1[3] = {0, 1, 4}, want_k2[3] = {3, 3, 4};
      for (int i = 0; i < 3; ++i)
        CHECK(lp.cons[i].dual_off == want_off[i] && lp.cons[i].p == want_p[i] && lp.cons[i].k1 == want_k1[i] && lp.cons[i].k2 == want_k2[i] &&
                  lp.cons[i].cp_off == -1 && lp.cons[i].cl_off == -1,
              "constraint %d: dual_off %lld p %d knots %d..%d", i, lp.cons[i].dual_off, lp.cons[i].p, lp.cons[i].k1, lp.cons[i].k2);
    }
  }
}

// ---- B. lower_constraint_params ---------------------------------------------------------------------------------------------------------
// The body of to_set_constraint_params_batch as it stood in trajopt_hip.hip before the lowering moved (verbatim but for `return fail(...)` ->
// `return 1`): shift[nz, B] zero-filled by the caller.
static int reference_constraint_params(const DevCon& ci, int n, int nz, int B, const double* params, std::vector<double>& shift) {
  const int p = ci.p;
  if (ci.d.kind == TO_CON_GOAL) {
    for (int b = 0; b < B; ++b)
      for (int r = 0; r < p; ++r) shift[(size_t)(ci.d.inds[r] - 1) + (size_t)nz * b] = params[r + (size_t)p * b] - ci.d.params[r];
  } else {
    // A z[inds] - (b + db) = A (z[inds] - dz) - b with the minimum-norm dz = A'(A A')^-1 db: needs linearly independent rows
    const int D = ci.d.n_inds;
    const double* A = ci.d.params;          // p x D, column-major
    const double* b0 = ci.d.params + (size_t)p * D;
    std::vector<double> G((size_t)p * p, 0.0), Lc((size_t)p * p, 0.0), w(p), y(p);
    double gmax = 0.0;
    for (int i = 0; i < p; ++i)
      for (int j = 0; j < p; ++j) { double t = 0.0; for (int c = 0; c < D; ++c) t += A[i + (size_t)p * c] * A[j + (size_t)p * c]; G[i + (size_t)p * j] = t; if (i == j) gmax = std::fmax(gmax, t); }
    for (int j = 0; j < p; ++j) {  // Cholesky of A A'
      double d = G[j + (size_t)p * j];
      for (int k = 0; k < j; ++k) d -= Lc[j + (size_t)p * k] * Lc[j + (size_t)p * k];
      if (!(d > 1e-12 * gmax)) return 1;
      Lc[j + (size_t)p * j] = std::sqrt(d);
      for (int i = j + 1; i < p; ++i) {
        double t = G[i + (size_t)p * j];
        for (int k = 0; k < j; ++k) t -= Lc[i + (size_t)p * k] * Lc[j + (size_t)p * k];
        Lc[i + (size_t)p * j] = t / Lc[j + (size_t)p * j];
      }
    }
    for (int b = 0; b < B; ++b) {
      for (int i = 0; i < p; ++i) { double t = params[i + (size_t)p * b] - b0[i]; for (int k = 0; k < i; ++k) t -= Lc[i + (size_t)p * k] * y[k]; y[i] = t / Lc[i + (size_t)p * i]; }
      for (int i = p - 1; i >= 0; --i) { double t = y[i]; for (int k = i + 1; k < p; ++k) t -= Lc[k + (size_t)p * i] * w[k]; w[i] = t / Lc[i + (size_t)p * i]; }
      for (int c = 0; c < D; ++c) { double t = 0.0; for (int i = 0; i < p; ++i) t += A[i + (size_t)p * c] * w[i]; shift[(size_t)(ci.d.inds[c] - 1) + (size_t)nz * b] += t; }
    }
    (void)n;
  }
  return 0;
}
static to_constraint_desc linear_con(int p, const std::vector<int>& inds, const std::vector<double>& A /* p x D, column-major */) {
  const int D = (int)inds.size();
  to_constraint_desc c;
  std::memset(&c, 0, sizeof(c));
  c.kind = TO_CON_LINEAR; c.sense = TO_CONE_ZERO; c.k_first = 1; c.k_last = 4; c.n_inds = D; c.n_params = p * (D + 1);
  for (int i = 0; i < D; ++i) c.inds[i] = inds[i];
  for (int i = 0; i < p * D; ++i) c.params[i] = A[i];
  for (int i = 0; i < p; ++i) c.params[p * D + i] = 0.5 - 0.125 * i;
  return c;
}
static double g_max_residual = 0.0;
// max over trajectories and rows of |A shift[inds] - (params_b - b0)| (GOAL: A = I), and the largest |shift| off inds
static void residuals(const DevCon& ci, int nz, int B, const double* params, const std::vector<double>& shift, double* res, double* off) {
  const int p = ci.p, D = ci.d.n_inds;
  *res = *off = 0.0;
  for (int b = 0; b < B; ++b) {
    for (int r = 0; r < p; ++r) {
      double t = 0.0, want;
      if (ci.d.kind == TO_CON_GOAL) { t = shift[(size_t)(ci.d.inds[r] - 1) + (size_t)nz * b]; want = params[r + (size_t)p * b] - ci.d.params[r]; }
      else {
        for (int c = 0; c < D; ++c) t += ci.d.params[r + (size_t)p * c] * shift[(size_t)(ci.d.inds[c] - 1) + (size_t)nz * b];
        want = params[r + (size_t)p * b] - ci.d.params[(size_t)p * D + r];
      }
      *res = std::fmax(*res, std::fabs(t - want));
    }
    for (int e = 0; e < nz; ++e) {
      bool on = false;
      for (int c = 0; c < D; ++c) on = on || ci.d.inds[c] - 1 == e;
      if (!on) *off = std::fmax(*off, std::fabs(shift[(size_t)e + (size_t)nz * b]));
    }
  }
}
static void params_case(const char* what, const to_constraint_desc& d) {
  const int n = 4, m = 1, nz = n + m, N = 5;
  DevCon ci;
  if (validate_constraint(n, m, N, d, &ci) != TO_OK) { CHECK(false, "%s: descriptor refused (%s)", what, g_err.c_str()); return; }
  for (int B : {1, 3, 65}) {
    std::vector<double> params((size_t)ci.p * B);
    for (double& v : params) v = next_value();
    std::vector<double> want((size_t)nz * B, 0.0), got(3, -1.0);
    const int ref_rc = reference_constraint_params(ci, n, nz, B, params.data(), want);
    const int rc = lower_constraint_params(ci, nz, B, params.data(), &got);
    CHECK(ref_rc == 0 && rc == TO_OK, "%s B %d: rc %d / %d (%s)", what, B, ref_rc, rc, g_err.c_str());
    CHECK(got.size() == want.size() && std::memcmp(got.data(), want.data(), sizeof(double) * want.size()) == 0, "%s B %d: differs from the loop it replaced", what, B);
    if (got.size() != want.size()) continue;
    double res_ref, off_ref, res, off;
    residuals(ci, nz, B, params.data(), want, &res_ref, &off_ref);
    residuals(ci, nz, B, params.data(), got, &res, &off);
    CHECK(res <= res_ref && off == 0.0, "%s B %d: residual %.3g (the replaced loop: %.3g), off inds %.3g", what, B, res, res_ref, off);
    CHECK(res_ref < 1e-9, "%s B %d: the reference itself misses the property by %.3g", what, B, res_ref);
    g_max_residual = std::fmax(g_max_residual, res);
  }
}
static int params_refusal(const char* name, const to_constraint_desc& d, bool must_agree_with_reference = true) {
  const int n = 4, m = 1, nz = n + m, N = 5, B = 3;
  DevCon ci;
  if (validate_constraint(n, m, N, d, &ci) != TO_OK) { CHECK(false, "%s: descriptor refused (%s)", name, g_err.c_str()); return TO_OK; }
  std::vector<double> params((size_t)ci.p * B, 0.75), got(2, 7.0), want((size_t)nz * B, 0.0);
  g_err.clear();
  const int rc = lower_constraint_params(ci, nz, B, params.data(), &got);
  if (rc != TO_OK) CHECK(got.size() == 2 && got[0] == 7.0 && got[1] == 7.0, "%s: the output was touched by a refused call", name);
  if (must_agree_with_reference) CHECK((reference_constraint_params(ci, n, nz, B, params.data(), want) != 0) == (rc != TO_OK), "%s: the replaced loop decides otherwise", name);
  report(name, rc);
  return rc;
}
static void constraint_params_cases() {
  params_case("goal p=1", goal_x(5, {3}));
  params_case("goal p=n", goal_x(5, {4, 1, 3, 2}));
  auto A = [](int p, int D) { std::vector<double> a((size_t)p * D); for (double& v : a) v = next_value(); return a; };
  params_case("linear (1, 1)", linear_con(1, {4}, A(1, 1)));
  params_case("linear (1, 3)", linear_con(1, {5, 1, 3}, A(1, 3)));
  params_case("linear (2, 3)", linear_con(2, {5, 1, 3}, A(2, 3)));
  params_case("linear (3, 3)", linear_con(3, {2, 5, 4}, A(3, 3)));
  params_refusal("params_kind", bound_u(1, 4, 3.0), false);  // (the replaced loop had this check ahead of its body)
  params_refusal("params_equal_rows", linear_con(2, {5, 1, 3}, {1.0, 1.0, 2.0, 2.0, 2.0, 2.0}));
  // row 1 = 1e-7 row 0 + delta (2, -1, 0): the second pivot is 5 delta^2 against 1e-12 |row 0|^2 = 9e-12
  auto nearly = [](double delta) { return linear_con(2, {5, 1, 3}, {1.0, 1e-7 + 2.0 * delta, 2.0, 2e-7 - delta, 2.0, 2e-7}); };
  CHECK(params_refusal("params_below_threshold", nearly(1.0e-6)) == TO_ERR_UNSUPPORTED, "5e-12 is below 9e-12");
  CHECK(params_refusal("params_above_threshold", nearly(1.5e-6)) == TO_OK, "1.125e-11 is above 9e-12");
}

// ---- C. cost_linear_delta / cost_linear_zero --------------------------------------------------------------------------------------------
static void cost_linear_cases() {
  const int n = 4, m = 2;
  to_cost_desc c;
  std::memset(&c, 0, sizeof(c));
  c.kind = TO_COST_DIAGONAL;
  for (int i = 0; i < n; ++i) c.q[i] = next_value();
  for (int j = 0; j < m; ++j) c.r[j] = next_value();
  for (int B : {1, 65}) {
    std::vector<double> q((size_t)n * B), r((size_t)m * B), dq(1, 7.0), dr(1, 7.0);
    for (double& v : q) v = next_value();
    for (double& v : r) v = next_value();
    CHECK(cost_linear_delta(c, n, m, B, q.data(), r.data(), &dq, &dr) == TO_OK, "B %d: both", B);
    CHECK(dq.size() == q.size() && dr.size() == r.size(), "B %d: sizes", B);
    for (int b = 0; b < B && dq.size() == q.size(); ++b) for (int i = 0; i < n; ++i) CHECK(dq[i + (size_t)n * b] == q[i + (size_t)n * b] - c.q[i], "B %d: dq[%d, %d]", B, i, b);
    for (int b = 0; b < B && dr.size() == r.size(); ++b) for (int j = 0; j < m; ++j) CHECK(dr[j + (size_t)m * b] == r[j + (size_t)m * b] - c.r[j], "B %d: dr[%d, %d]", B, j, b);
    std::vector<double> keep_q(2, 7.0), keep_r(2, 7.0);
    CHECK(cost_linear_delta(c, n, m, B, nullptr, r.data(), &keep_q, &dr) == TO_OK && keep_q == std::vector<double>(2, 7.0) && dr.size() == r.size(), "B %d: q NULL leaves dq alone", B);
    CHECK(cost_linear_delta(c, n, m, B, q.data(), nullptr, &dq, &keep_r) == TO_OK && keep_r == std::vector<double>(2, 7.0) && dq.size() == q.size(), "B %d: r NULL leaves dr alone", B);
    std::vector<double> zero(3, 1.0);
    cost_linear_zero(n, m, B, &zero);
    CHECK(zero == std::vector<double>((size_t)(n + m) * B, 0.0), "B %d: zero rows", B);
  }
  std::vector<double> q(n * 3, 1.0), dq(2, 7.0), dr(2, 7.0);
  auto refusal = [&](const char* name, const to_cost_desc& cost, const double* qq) {
    g_err.clear();
    const int rc = cost_linear_delta(cost, n, m, 3, qq, nullptr, &dq, &dr);
    CHECK(dq == std::vector<double>(2, 7.0) && dr == std::vector<double>(2, 7.0), "%s: the output was touched by a refused call", name);
    report(name, rc);
  };
  to_cost_desc eq = c;
  eq.kind = TO_COST_ERROR_QUADRATIC;
  refusal("linear_both_null", c, nullptr);
  refusal("linear_error_quadratic", eq, q.data());
  refusal("order_null_before_kind", eq, nullptr);
}

// ---- D. the plant-parameter rule --------------------------------------------------------------------------------------------------------
static void plant_cases() {
  const int n_keys = N_MODEL_KEYS;  // -DN_MODEL_KEYS=<handle.h's>: tests/test_problem_lower_host.py reads it from that header
  double mp[16];
  for (int i = 0; i < 16; ++i) mp[i] = 1.0 + i;
  auto selects = [](int key, int i) {
    if (key <= 2 || key == 7) return i == 1;
    if (key >= 4 && key <= 6) return i == 10;
    if (key == 9 || key == 10) return i == 1 || i == 15;
    if (key == 11) return i == 15;
    return false;  // 3: the Cartpole has no such entry
  };
  const std::string changed = " change the model's dimensions or attitude representation";
  for (int key = 0; key < n_keys; ++key)
    for (int need_finite = 0; need_finite < 2; ++need_finite) {
      const std::string where = need_finite ? " of trajectory 3" : "";
      g_err.clear();
      const int same = validate_plant_params("who", key, mp, mp, need_finite != 0, where);
      if (key == 8) CHECK(same == TO_ERR_ARGUMENT && g_err == "who: a model vector takes no plant_params (its models live in the step table)", "key 8: %d %s", same, g_err.c_str());
      else CHECK(same == TO_OK, "key %d: the problem's own parameters refused (%s)", key, g_err.c_str());
      for (int i = 0; i < 16; ++i) {
        double pp[16];
        std::memcpy(pp, mp, sizeof(pp));
        pp[i] = mp[i] + 1.0;
        g_err.clear();
        int rc = validate_plant_params("who", key, mp, pp, need_finite != 0, where);
        if (key == 8) CHECK(rc == TO_ERR_ARGUMENT && g_err.find("a model vector takes no plant_params") != std::string::npos, "key 8 entry %d", i);
        else if (selects(key, i))
          CHECK(rc == TO_ERR_ARGUMENT && g_err == std::string("who: ") + (need_finite ? "the parameters of trajectory 3" : "plant_params") + changed, "key %d entry %d: %d %s", key, i, rc, g_err.c_str());
        else CHECK(rc == TO_OK && plant_params_compatible(key, mp, pp), "key %d entry %d refused (%s)", key, i, g_err.c_str());
        if (key != 8) CHECK(plant_params_compatible(key, mp, pp) == !selects(key, i), "key %d entry %d: the predicate", key, i);
        if (key == 8 || selects(key, i)) continue;
        pp[i] = NaN;  // a NaN in an entry that selects nothing
        g_err.clear();
        rc = validate_plant_params("who", key, mp, pp, need_finite != 0, where);
        if (need_finite) CHECK(rc == TO_ERR_ARGUMENT && g_err == "who: entry " + std::to_string(i) + " of trajectory 3 is not finite", "key %d entry %d NaN: %d %s", key, i, rc, g_err.c_str());
        else CHECK(rc == TO_OK, "key %d entry %d NaN refused without need_finite (%s)", key, i, g_err.c_str());
      }
    }
  double pp[16];
  auto refusal = [&](const char* name, const char* who, int key, bool need_finite, const std::string& where) {
    g_err.clear();
    report(name, validate_plant_params(who, key, mp, pp, need_finite, where));
  };
  std::memcpy(pp, mp, sizeof(pp)); pp[6] = Inf;
  refusal("plant_setter_not_finite", "to_set_model_params_batch", 4, true, " of trajectory 2");
  pp[10] = 2.0;
  refusal("order_not_finite_before_changed", "to_set_model_params_batch", 4, true, " of trajectory 2");
  pp[6] = mp[6];
  refusal("plant_setter_changed", "to_set_model_params_batch", 4, true, " of trajectory 2");
  refusal("plant_policy_changed", "to_policy_rollout", 4, false, "");
  refusal("plant_policy_sample_changed", "to_policy_rollout", 4, false, " of sample (b = 1, s = 2)");
  refusal("plant_model_vector", "to_policy_rollout", 8, false, "");
  std::memcpy(pp, mp, sizeof(pp)); pp[3] = NaN;
  refusal("plant_policy_nan_passes", "to_policy_rollout", 4, false, "");
}

int main() {
  problem_cases();
  constraint_params_cases();
  cost_linear_cases();
  plant_cases();
  printf("max_residual %.3g\n", g_max_residual);
  printf("fails %d\n", fails);
  return fails ? 1 : 0;
}
