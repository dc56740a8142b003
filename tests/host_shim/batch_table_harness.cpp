// Compiles the one host routine behind every per-trajectory table with a spare tile (csrc/desc_lower.h tile_rows / tiled_len: DevProblem::pm,
// dtb, cl, gw, ga) as a program of its own (test infrastructure; tests/test_batch_table_host.py, which also builds it with
// -fsanitize=address,undefined).  Checks, lane by lane against a restatement of the layout rule — entry e of trajectory b at
// ((b >> 6) * L + e) * 64 + (b & 63); every lane behind the batch and the whole spare tile on the shared value of its row —
//   the routine itself over a grid of (L, B), with values and with values == NULL;
//   the image of pm (16 rows, the shared plant) and of cl (the rows of every constraint: constraint_limits_bases / _shared / _values) at B = 65;
// and prints, for fixed inputs given by formulas,
//   hash <table> <B> <fnv1a-64 of the image's bytes>     for the five tables at B = 1, 64, 65, 300 (held to the hashes recorded from the loops
//                                                        this routine replaced), then "checks <n> fails <n>".
#include "desc_lower.h"

#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

static long long fails = 0, checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static uint64_t fnv1a(const std::vector<double>& v) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char* p = (const unsigned char*)v.data();
  for (size_t i = 0; i < v.size() * sizeof(double); ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

// the layout rule, restated: want(b, e) for every trajectory slot of every tile, the spare one included
template <class Want>
static void check_image(const char* what, const std::vector<double>& tiled, size_t L, int B, int Bp, Want want) {
  CHECK(tiled.size() == ((size_t)Bp / 64 + 1) * L * 64 && tiled.size() == tiled_len(L, Bp), "%s L %zu B %d: %zu doubles", what, L, B, tiled.size());
  if (tiled.size() != ((size_t)Bp / 64 + 1) * L * 64) return;
  for (size_t b = 0; b < (size_t)Bp + 64; ++b)
    for (size_t e = 0; e < L; ++e) {
      const double v = tiled[((b >> 6) * L + e) * 64 + (b & 63)], w = want(b, e);
      CHECK(v == w, "%s L %zu B %d: entry %zu of %s %zu holds %.17g, not %.17g", what, L, B, e, b < (size_t)B ? "trajectory" : b < (size_t)Bp ? "padding lane" : "spare lane", b, v, w);
    }
}

static void grid_case(size_t L, int B) {
  const int Bp = (B + 63) / 64 * 64;
  std::vector<double> values(L * B), shared(L), tiled(3, -1.0);
  for (size_t e = 0; e < L; ++e) shared[e] = -1.0 - (double)e;                                           // every value distinct
  for (int b = 0; b < B; ++b) for (size_t e = 0; e < L; ++e) values[L * b + e] = 1.0 + (double)(L * b + e);
  tile_rows(L, B, Bp, values.data(), shared.data(), &tiled);
  check_image("values", tiled, L, B, Bp, [&](size_t b, size_t e) { return b < (size_t)B ? values[L * b + e] : shared[e]; });
  std::vector<double> back(L * B);   // the round trip through the address the kernels form
  for (int b = 0; b < B; ++b) for (size_t e = 0; e < L; ++e) back[L * b + e] = tiled[(((size_t)(b >> 6)) * L + e) * 64 + (b & 63)];
  CHECK(back == values, "L %zu B %d: round trip", L, B);
  tile_rows(L, B, Bp, nullptr, shared.data(), &tiled);
  check_image("null", tiled, L, B, Bp, [&](size_t, size_t e) { return shared[e]; });
}

// ---- fixed inputs, by formula ----
static const double INF = std::numeric_limits<double>::infinity();
static const int GN = 4, GM = 2, GNC = 3, GSTEPS = 31;
static std::vector<to_cost_desc> golden_costs() {
  std::vector<to_cost_desc> c(GNC);
  for (int ci = 0; ci < GNC; ++ci) {
    std::memset(&c[ci], 0, sizeof(to_cost_desc));
    c[ci].kind = ci == 1 ? TO_COST_DIAGONAL_QUAT : TO_COST_DIAGONAL;
    for (int i = 0; i < GN; ++i) c[ci].Q[i] = 10.0 * (ci + 1) + i;
    for (int j = 0; j < GM; ++j) c[ci].R[j] = 0.1 * (ci + 1) + 0.01 * j;
    for (int i = 0; i < 4; ++i) c[ci].q_ref[i] = 0.25 * (ci + 1) + 0.01 * i;
  }
  return c;
}
static void golden_plants(int B, double* mp, std::vector<double>* params) {
  for (int i = 0; i < 16; ++i) mp[i] = 0.5 + 0.25 * i;
  params->resize((size_t)16 * B);
  for (int b = 0; b < B; ++b) for (int i = 0; i < 16; ++i) (*params)[16 * (size_t)b + i] = 1.0 + 0.001 * i + 0.01 * b;
}
static void golden_steps(int B, std::vector<double>* shared, std::vector<double>* dt) {
  const int L = GSTEPS - 1;
  shared->resize(L); dt->resize((size_t)L * B);
  for (int k = 0; k < L; ++k) (*shared)[k] = 0.05 + 1e-3 * k;
  for (int b = 0; b < B; ++b) for (int k = 0; k < L; ++k) (*dt)[k + (size_t)L * b] = 0.01 * (b + 1) + 1e-4 * (k + 1);
}
static void golden_weights(int B, const std::vector<to_cost_desc>& c, std::vector<double>* values) {
  std::vector<double> Q((size_t)GN * B), R((size_t)GM * B);
  for (int b = 0; b < B; ++b) { for (int i = 0; i < GN; ++i) Q[i + (size_t)GN * b] = 1000.0 * b + i; for (int j = 0; j < GM; ++j) R[j + (size_t)GM * b] = -1000.0 * b - j; }
  cost_weights_fill(GN, GM, B, c.data(), GNC, values);
  cost_weights_store(GN, GM, B, GNC, 1, Q.data(), nullptr, values);
  cost_weights_store(GN, GM, B, GNC, 2, nullptr, R.data(), values);
}
static void golden_attitudes(int B, const std::vector<to_cost_desc>& c, std::vector<double>* values) {
  cost_attitude_fill(B, c.data(), GNC, values);
  for (int b = 0; b < B; ++b) for (int i = 0; i < 4; ++i) (*values)[(size_t)4 * GNC * b + 4 * 1 + i] = 1000.0 * b + i;
}
// constraint 0: a BoundConstraint with mixed upper and lower rows (p = 6); constraint 1: an SOC NormConstraint on the controls (p = 3)
static std::vector<DevCon> golden_cons() {
  const int N = 11;
  std::vector<DevCon> cons(2);
  to_constraint_desc d{};
  d.kind = TO_CON_BOUND; d.sense = TO_CONE_NEGATIVE_ORTHANT; d.k_first = 1; d.k_last = N - 1; d.n_params = 2 * (GN + GM);
  const double zmax[6] = {INF, INF, INF, 0.7, 1.2, 1.2}, zmin[6] = {-0.5, -INF, -INF, -INF, -1.2, -1.2};
  for (int i = 0; i < GN + GM; ++i) { d.params[i] = zmax[i]; d.params[GN + GM + i] = zmin[i]; }
  int rc = validate_constraint(GN, GM, N, d, &cons[0]);
  CHECK(rc == TO_OK && cons[0].p == 6, "bound: rc %d (%s)", rc, g_err.c_str());
  to_constraint_desc s{};
  s.kind = TO_CON_NORM; s.sense = TO_CONE_SECOND_ORDER; s.k_first = 1; s.k_last = N - 1; s.n_inds = GM; s.n_params = 1; s.params[0] = 6.0;
  for (int i = 0; i < GM; ++i) s.inds[i] = GN + i + 1;
  rc = validate_constraint(GN, GM, N, s, &cons[1]);
  CHECK(rc == TO_OK && cons[1].p == 3, "cone: rc %d (%s)", rc, g_err.c_str());
  return cons;
}
static void golden_bound_limits(int B, std::vector<double>* lim) {   // [6, B]: three upper rows, three lower rows
  lim->resize((size_t)6 * B);
  for (int b = 0; b < B; ++b) {
    double* l = lim->data() + (size_t)6 * b;
    l[0] = 0.6 + 0.001 * b; l[1] = 1.0 + 0.002 * b; l[2] = 1.5 + 0.003 * b; l[3] = -0.5 - 0.001 * b; l[4] = -0.9 - 0.002 * b; l[5] = -1.4 - 0.003 * b;
  }
}
// the image of cl as the library builds it (trajopt_hip.hip upload_constraint_limits, without the copy)
static int limits_image(const std::vector<DevCon>& cons, const std::vector<std::vector<double>>& given, int B, int Bp, std::vector<int>* base, std::vector<double>* tiled) {
  std::vector<double> shared, values;
  const int n_cl = constraint_limits_bases(cons, base);
  constraint_limits_shared(cons, *base, n_cl, &shared);
  if (int r = constraint_limits_values(cons, given, *base, shared, B, &values)) return r;
  tile_rows(shared.size(), B, Bp, values.data(), shared.data(), tiled);
  return TO_OK;
}

static void plants_and_limits() {
  const int B = 65, Bp = 128;
  double mp[16];
  std::vector<double> params, tiled;
  golden_plants(B, mp, &params);
  tile_rows(16, B, Bp, params.data(), mp, &tiled);
  check_image("pm", tiled, 16, B, Bp, [&](size_t b, size_t e) { return b < (size_t)B ? params[16 * b + e] : mp[e]; });
  tile_rows(16, B, Bp, nullptr, mp, &tiled);   // a handle that carries time steps only: the shared plant for every trajectory
  check_image("pm shared", tiled, 16, B, Bp, [&](size_t, size_t e) { return mp[e]; });

  const std::vector<DevCon> cons = golden_cons();
  std::vector<int> base;
  std::vector<double> bound, cone(B);
  golden_bound_limits(B, &bound);
  for (int b = 0; b < B; ++b) cone[b] = 4.0 + 0.05 * b;
  // what row r of constraint i is for trajectory slot b, from the setter's arguments and the descriptors alone
  auto want = [&](bool bound_set, bool cone_set) {
    return [&, bound_set, cone_set](size_t b, size_t e) {
      const bool live = b < (size_t)B;
      if (e < 6) return live && bound_set ? bound[e + 6 * b] : cons[0].soff[e];
      const size_t r = e - 6;
      return live && cone_set ? (r == 2 ? cone[b] : 0.0) : cons[1].soff[r];
    };
  };
  int rc = limits_image(cons, {bound, {}}, B, Bp, &base, &tiled);
  CHECK(rc == TO_OK && base.size() == 2 && base[0] == 0 && base[1] == 6, "cl, the bound flagged: rc %d (%s)", rc, g_err.c_str());
  check_image("cl bound", tiled, 9, B, Bp, want(true, false));
  rc = limits_image(cons, {{}, cone}, B, Bp, &base, &tiled);
  CHECK(rc == TO_OK, "cl, the cone flagged: rc %d (%s)", rc, g_err.c_str());
  check_image("cl cone", tiled, 9, B, Bp, want(false, true));
  CHECK(cons[1].soff[2] == 6.0 && cons[0].soff[0] == 0.7 && cons[0].soff[3] == -0.5, "the shared rows are the descriptors' offsets");
  // a refusal of one constraint's limits reaches the caller (the entry point has refused them before; the table is not built)
  cone[7] = -1.0;
  std::vector<double> untouched(2, 7.0);
  rc = limits_image(cons, {bound, cone}, B, Bp, &base, &untouched);
  CHECK(rc == TO_ERR_ASSERTION && untouched.size() == 2 && untouched[0] == 7.0, "a refused limit: rc %d", rc);
}

static void hashes() {
  const auto costs = golden_costs();
  const auto cons = golden_cons();
  for (int B : {1, 64, 65, 300}) {
    const int Bp = (B + 63) / 64 * 64;
    std::vector<double> img, shared, values;
    double mp[16];
    golden_plants(B, mp, &values);
    tile_rows(16, B, Bp, values.data(), mp, &img);
    printf("hash pm %d %016llx\n", B, (unsigned long long)fnv1a(img));
    std::vector<int> base;
    std::vector<std::vector<double>> given(2);
    golden_bound_limits(B, &given[0]);
    const int rc = limits_image(cons, given, B, Bp, &base, &img);
    CHECK(rc == TO_OK, "cl at B %d: rc %d (%s)", B, rc, g_err.c_str());
    printf("hash cl %d %016llx\n", B, (unsigned long long)fnv1a(img));
    golden_steps(B, &shared, &values);
    CHECK(lower_time_steps(GSTEPS, B, Bp, values.data(), shared.data(), &img) == TO_OK, "dtb at B %d: %s", B, g_err.c_str());
    printf("hash dtb %d %016llx\n", B, (unsigned long long)fnv1a(img));
    golden_weights(B, costs, &values);
    cost_weights_shared(GN, GM, costs.data(), GNC, &shared);
    tile_rows(shared.size(), B, Bp, values.data(), shared.data(), &img);
    printf("hash gw %d %016llx\n", B, (unsigned long long)fnv1a(img));
    golden_attitudes(B, costs, &values);
    cost_attitude_shared(costs.data(), GNC, &shared);
    tile_rows(shared.size(), B, Bp, values.data(), shared.data(), &img);
    printf("hash ga %d %016llx\n", B, (unsigned long long)fnv1a(img));
  }
}

int main() {
  for (size_t L : {1, 2, 16, 50})
    for (int B : {1, 6, 63, 64, 65, 70, 128, 300}) grid_case(L, B);
  plants_and_limits();
  hashes();
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
