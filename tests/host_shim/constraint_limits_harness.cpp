// Compiles the host-only lowering of per-trajectory constraint limits (csrc/desc_lower.h: constraint_limits_q, lower_constraint_limits,
// shared_constraint_limits — what to_set_constraint_limits_batch / to_get_... run before anything reaches the device) as a program of its
// own (test infrastructure; tests/test_constraint_limits_host.py, which also builds it with -fsanitize=address,undefined).  Prints
//   rows <name> p <p> : one line per trajectory and row, "b r idx sgn value" — the selector tables next to the lowered values, so that the
//                       test can restate row r of trajectory b as sgn * (z[idx] - value) (value itself for idx = -1) and hold it to the oracle;
//   case <name> code <c> msg <text> : every refusal, with the error class and the message.
#include "desc_lower.h"

#include <cstdio>
#include <limits>
#include <string>
#include <vector>

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

static const double INF = std::numeric_limits<double>::infinity();
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

static to_constraint_desc bound_desc(int n, int m, const std::vector<double>& zmax, const std::vector<double>& zmin, int N) {
  to_constraint_desc d{};
  d.kind = TO_CON_BOUND; d.sense = TO_CONE_NEGATIVE_ORTHANT; d.k_first = 1; d.k_last = N - 1; d.n_params = 2 * (n + m);
  for (int i = 0; i < n + m; ++i) { d.params[i] = zmax[i]; d.params[n + m + i] = zmin[i]; }
  return d;
}
static to_constraint_desc norm_desc(int n, int m, double val, int sense, int N) {
  to_constraint_desc d{};
  d.kind = TO_CON_NORM; d.sense = sense; d.k_first = 1; d.k_last = N - 1; d.n_inds = m; d.n_params = 1; d.params[0] = val;
  for (int i = 0; i < m; ++i) d.inds[i] = n + i + 1;
  return d;
}
static void print_rows(const char* name, const DevCon& c, int B, const std::vector<double>& rows) {
  printf("rows %s p %d\n", name, c.p);
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < c.p; ++r) printf("%d %d %d %g %.17g\n", b, r, c.sidx[r], c.ssgn[r], rows[r + (size_t)c.p * b]);
}
static void refusal(const char* name, const DevCon& c, int B, const std::vector<double>& lim) {
  std::vector<double> rows(3, 123.0);
  g_err.clear();
  const int rc = lower_constraint_limits(c, B, lim.data(), &rows);
  printf("case %s code %d msg %s\n", name, rc, g_err.c_str());
}

int main() {
  const int n = 4, m = 2, N = 11;
  DevCon mixed, ctrl, soc, quad, goal;
  // the bound of the double-integrator fleet: state and control rows, finite and infinite entries mixed
  int rc = validate_constraint(n, m, N, bound_desc(n, m, {INF, INF, INF, 0.7, 1.2, 1.2}, {-0.5, -INF, -INF, -INF, -1.2, -1.2}, N), &mixed);
  CHECK(rc == TO_OK && mixed.p == 6 && mixed.cl_off == -1 && mixed.cp_off == -1, "mixed bound: rc %d p %d", rc, mixed.p);
  rc = validate_constraint(n, m, N, bound_desc(n, m, {INF, INF, INF, INF, 3.0, INF}, {-INF, -INF, -INF, -INF, -3.0, -INF}, N), &ctrl);
  CHECK(rc == TO_OK && ctrl.p == 2, "control bound: rc %d p %d", rc, ctrl.p);
  rc = validate_constraint(n, m, N, norm_desc(n, m, 6.0, TO_CONE_SECOND_ORDER, N), &soc);
  CHECK(rc == TO_OK && soc.p == m + 1 && soc.fast == 2, "cone: rc %d p %d fast %d", rc, soc.p, soc.fast);
  rc = validate_constraint(n, m, N, norm_desc(n, m, 6.0, TO_CONE_NEGATIVE_ORTHANT, N), &quad);
  CHECK(rc == TO_OK && quad.p == 1 && !quad.selector, "quadratic norm: rc %d", rc);
  {
    to_constraint_desc d{};
    d.kind = TO_CON_GOAL; d.sense = TO_CONE_ZERO; d.k_first = d.k_last = N; d.n_inds = d.n_params = n;
    for (int i = 0; i < n; ++i) d.inds[i] = i + 1;
    rc = validate_constraint(n, m, N, d, &goal);
    CHECK(rc == TO_OK, "goal: rc %d", rc);
  }
  int q = -1;
  CHECK(constraint_limits_q(mixed, &q) == TO_OK && q == 6, "q of the mixed bound: %d", q);
  CHECK(constraint_limits_q(soc, &q) == TO_OK && q == 1, "q of the cone: %d", q);
  // ---- lowering: three trajectories each
  const int B = 3;
  std::vector<double> rows;
  const std::vector<double> lim_mixed = {0.6, 1.0, 1.5, -0.5, -0.9, -1.4,   0.85, 0.8, 1.6, -0.5, -1.6, -0.8,   0.7, 1.2, 1.2, -0.5, -1.2, -1.2};
  rc = lower_constraint_limits(mixed, B, lim_mixed.data(), &rows);
  CHECK(rc == TO_OK && rows.size() == (size_t)6 * B, "mixed bound lowering: rc %d (%s)", rc, g_err.c_str());
  for (size_t i = 0; i < rows.size() && i < lim_mixed.size(); ++i) CHECK(rows[i] == lim_mixed[i], "mixed bound: row value %zu", i);
  print_rows("mixed", mixed, B, rows);
  const std::vector<double> lim_soc = {4.5, 7.5, 0.0};
  rc = lower_constraint_limits(soc, B, lim_soc.data(), &rows);
  CHECK(rc == TO_OK && rows.size() == (size_t)(m + 1) * B, "cone lowering: rc %d (%s)", rc, g_err.c_str());
  for (int b = 0; b < B; ++b) {
    for (int r = 0; r < m; ++r) CHECK(rows[r + (size_t)(m + 1) * b] == 0.0, "cone: selector row %d of trajectory %d carries an offset", r, b);
    CHECK(rows[m + (size_t)(m + 1) * b] == lim_soc[b], "cone: value of trajectory %d", b);
  }
  print_rows("cone", soc, B, rows);
  // ---- what the getter reports for a constraint on shared limits: the descriptor's values in the setter's layout
  double sh[8];
  shared_constraint_limits(mixed, 6, sh);
  const double want[6] = {0.7, 1.2, 1.2, -0.5, -1.2, -1.2};
  for (int i = 0; i < 6; ++i) CHECK(sh[i] == want[i], "shared limits of the mixed bound: entry %d = %g", i, sh[i]);
  shared_constraint_limits(soc, 1, sh);
  CHECK(sh[0] == 6.0, "shared value of the cone: %g", sh[0]);
  // ---- refusals
  const double nan = std::numeric_limits<double>::quiet_NaN();
  refusal("nonfinite_bound", ctrl, 2, {3.0, -3.0, INF, -3.0});
  refusal("nan_bound", ctrl, 2, {3.0, -3.0, 3.0, nan});
  refusal("nonfinite_cone", soc, 2, {6.0, INF});
  refusal("inverted_bound", ctrl, 3, {3.0, -3.0, 4.0, -4.0, -1.0, -0.5});
  refusal("inverted_mixed", mixed, 2, {0.6, 1.0, 1.5, -0.5, -0.9, -1.4,   0.85, 0.8, -1.0, -0.5, -1.6, -0.8});
  refusal("negative_cone", soc, 3, {6.0, 0.0, -0.1});
  refusal("quadratic_norm", quad, 1, {6.0});
  refusal("goal", goal, 1, {0.0});
  // (an upper row without a lower row of the same coordinate has nothing to be compared with: x4 <= -3 alone is a valid bound)
  rc = lower_constraint_limits(mixed, 1, std::vector<double>{-3.0, 1.0, 1.5, -0.5, -0.9, -1.4}.data(), &rows);
  CHECK(rc == TO_OK, "one-sided rows: rc %d (%s)", rc, g_err.c_str());
  // equal upper and lower bounds are allowed (src/constraints.jl:711: only max < min is refused)
  rc = lower_constraint_limits(ctrl, 1, std::vector<double>{2.0, 2.0}.data(), &rows);
  CHECK(rc == TO_OK, "equal bounds: rc %d (%s)", rc, g_err.c_str());
  printf("fails %d\n", fails);
  return fails ? 1 : 0;
}
