// Compiles csrc/k_track.h — the kernel of to_set_tracking_reference_batch / to_set_tracking_window — for the host and runs it thread by
// thread (test infrastructure; tests/test_tracking_reference_host.py builds this as a stand-alone program under AddressSanitizer + UBSan).
// Every array has exactly the size the entry points give it, so a row too far is a heap overflow the sanitizer reports; every element of gl
// is compared, as a 64-bit pattern, with the plain loop of the host recipe
//     diagonal kinds:  delta = (-(Q_i x_i)) - c.q[i]         QUADRATIC:  acc = Q[i,0] x_0; acc = acc + Q[i,j] x_j (ascending j); delta = (-acc) - c.q[i]
// at reference knot j = min(start_b - 1 + k, Nref - 1), likewise for the r rows — which, like the lanes behind B and the rows of a cost no
// knot uses, must be left untouched when the reference has no controls.
// Cases: (n, m, N) in {(2,1,4), (4,1,21), (13,4,15)} with diagonal kinds and (4,2,9) with dense QUADRATIC costs, B in {1, 64, 65, 130},
// Nref in {N, N+7}, starts {all 1, one per trajectory, some windows past the end}, Uref {given, NULL}, one and up to 32 row groups.
// Then the host-only validation of csrc/desc_lower.h: every refusal of the two entry points with its error class.
// Output: "checks <count> fails <count>".
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

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

static long long g_checks = 0, g_fails = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
// a finite double of moderate magnitude with a full mantissa (so that a fused multiply-add WOULD round differently), now and then a signed zero
static double next_value() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  if ((g_rng & 63) == 0) return (g_rng & 64) ? -0.0 : 0.0;
  uint64_t bits = (g_rng & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 8 + (g_rng >> 52) % 16) << 52);
  double v;
  std::memcpy(&v, &bits, sizeof v);
  return v;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static void expect(bool ok, const char* what, const std::string& where) {
  ++g_checks;
  if (ok) return;
  if (++g_fails <= 20) std::printf("FAIL %s: %s\n", what, where.c_str());
}

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

// the host recipe for one row: what to_set_cost_linear_batch stores when it is handed q_b = -Q x_ref (r_b = -R u_ref)
static double recipe(const to_cost_desc& c, bool state, int d, int r, const double* z /* [d] */) {
  const double* W = state ? c.Q : c.R;
  double acc;
  if (c.kind == TO_COST_QUADRATIC) {
    acc = W[r] * z[0];
    for (int col = 1; col < d; ++col) { const double p = W[r + d * col] * z[col]; acc = acc + p; }
  } else {
    acc = W[r] * z[r];
  }
  const double qb = -acc;
  return qb - (state ? c.q[r] : c.r[r]);
}

static void one_case(int n, int m, int N, int B, int Nref, int start_mode, bool with_u, bool dense, bool wide) {
  const int nz = n + m, tiles = (B + 63) / 64, n_costs = N + 1, Lr = Nref * nz, L = n_costs * nz;
  const std::string where = "n " + std::to_string(n) + " m " + std::to_string(m) + " N " + std::to_string(N) + " B " + std::to_string(B) + " Nref " +
                            std::to_string(Nref) + " starts " + std::to_string(start_mode) + " u " + std::to_string(with_u) + " dense " + std::to_string(dense) +
                            " wide " + std::to_string(wide);
  std::unique_ptr<to_cost_desc[]> costs(new to_cost_desc[n_costs]);
  for (int c = 0; c < n_costs; ++c) {
    std::memset(&costs[c], 0, sizeof(to_cost_desc));
    costs[c].kind = dense ? (c % 4 == 3 ? TO_COST_DIAGONAL : TO_COST_QUADRATIC) : (n == 13 && c % 2 ? TO_COST_DIAGONAL_QUAT : TO_COST_DIAGONAL);
    for (int i = 0; i < TO_MAX_N * TO_MAX_N; ++i) costs[c].Q[i] = next_value();
    for (int i = 0; i < TO_MAX_M * TO_MAX_M; ++i) costs[c].R[i] = next_value();
    for (int i = 0; i < TO_MAX_N; ++i) costs[c].q[i] = next_value();
    for (int i = 0; i < TO_MAX_M; ++i) costs[c].r[i] = next_value();
  }
  // every knot its own cost, not in knot order, one cost of the list unused
  std::unique_ptr<int[]> cost_index(new int[N]);
  for (int k = 0; k < N; ++k) cost_index[k] = (k * 3 + 1) % n_costs;  // injective for the shapes here (checked below)
  for (int k = 0; k < N; ++k)
    for (int l = k + 1; l < N; ++l) expect(cost_index[k] != cost_index[l], "harness: cost_index injective", where);
  std::unique_ptr<int[]> start(new int[B]);
  for (int b = 0; b < B; ++b)
    start[b] = start_mode == 0 ? 1 : start_mode == 1 ? 1 + b % (Nref - N + 1 > 1 ? Nref - N + 1 : 3) : 1 + (b * 5 + 2) % Nref;  // mode 2: up to Nref, windows past the end
  auto ref = filled((size_t)tiles * Lr * 64);
  auto gl = filled((size_t)tiles * L * 64);
  std::vector<double> gl_old(gl.get(), gl.get() + (size_t)tiles * L * 64);
  TrackArgs a;
  std::memset(&a, 0, sizeof a);
  a.n = n; a.m = m; a.N = N; a.B = B; a.Nref = Nref; a.with_u = with_u ? 1 : 0; a.n_costs = n_costs;
  a.ref = ref.get(); a.start = start.get(); a.cost_index = cost_index.get(); a.costs = costs.get(); a.gl = gl.get();
  const int rows = N * (with_u ? nz : n);
  run(a, (unsigned)tiles, (unsigned)(wide ? (rows < 32 ? rows : 32) : 1));
  auto tiled = [](const double* p, int Ld, int b, int e) { return p[((size_t)(b >> 6) * Ld + e) * 64 + (b & 63)]; };
  auto at = [&](bool ok, const char* what, int b, int k) {  // (the text is built for a failure only)
    if (ok) ++g_checks; else expect(false, what, where + " b " + std::to_string(b) + " k " + std::to_string(k));
  };
  std::vector<char> used(n_costs, 0);
  for (int k = 0; k < N; ++k) used[cost_index[k]] = 1;
  for (int b = 0; b < tiles * 64; ++b) {
    for (int c = 0; c < n_costs; ++c)
      if (b >= B || !used[c])
        for (int i = 0; i < nz; ++i) at(same_bits(tiled(gl.get(), L, b, c * nz + i), tiled(gl_old.data(), L, b, c * nz + i)), "untouched", b, c);
    if (b >= B) continue;
    for (int k = 0; k < N; ++k) {
      int j = start[b] - 1 + k;
      if (j > Nref - 1) j = Nref - 1;
      const int c = cost_index[k];
      double z[TO_MAX_N + TO_MAX_M];
      for (int i = 0; i < nz; ++i) z[i] = tiled(ref.get(), Lr, b, j * nz + i);
      for (int i = 0; i < n; ++i) at(same_bits(tiled(gl.get(), L, b, c * nz + i), recipe(costs[c], true, n, i, z)), "q row", b, k);
      for (int i = 0; i < m; ++i) {
        const double want = with_u ? recipe(costs[c], false, m, i, z + n) : tiled(gl_old.data(), L, b, c * nz + n + i);
        at(same_bits(tiled(gl.get(), L, b, c * nz + n + i), want), with_u ? "r row" : "r row kept", b, k);
      }
    }
  }
}

// ---- the refusals (desc_lower.h) ----------------------------------------------------------------------------------------------------
static void refusal(int got, int want, const char* text, const char* what) {
  expect(got == want, what, "error class " + std::to_string(got) + " (want " + std::to_string(want) + "): " + g_err);
  if (text) expect(g_err.find(text) != std::string::npos, what, "message '" + g_err + "' lacks '" + text + "'");
}

static void validation_cases() {
  const int n = 4, m = 1, N = 5, B = 3, Nref = 8;
  std::vector<to_cost_desc> costs(N);
  for (auto& c : costs) { std::memset(&c, 0, sizeof c); c.kind = TO_COST_DIAGONAL; }
  std::vector<int> idx = {0, 1, 2, 3, 4};
  std::vector<double> X((size_t)n * Nref * B, 0.5), U((size_t)m * Nref * B, 0.25);
  std::vector<int32_t> start = {1, 2, 4};
  TrackFacts f{3, "Cartpole", n, m, N, B, costs.data(), N, idx.data(), false, 0, 0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // accepted: with and without controls and starts, both end modes
  refusal(validate_tracking_reference(f, Nref, X.data(), U.data(), start.data(), TO_TRACK_END_REFUSE), TO_OK, nullptr, "accepted");
  refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, nullptr, TO_TRACK_END_HOLD), TO_OK, nullptr, "accepted without U and starts");
  refusal(validate_tracking_reference(f, N, X.data(), nullptr, nullptr, TO_TRACK_END_REFUSE), TO_OK, nullptr, "accepted at Nref = N");
  // TO_ERR_NULL
  refusal(validate_tracking_reference(f, Nref, nullptr, U.data(), start.data(), 0), TO_ERR_NULL, "Xref is NULL", "Xref NULL");
  // TO_ERR_ARGUMENT
  refusal(validate_tracking_reference(f, 0, X.data(), nullptr, nullptr, 0), TO_ERR_ARGUMENT, "Nref must be >= 1", "Nref < 1");
  refusal(validate_tracking_reference(f, -3, X.data(), nullptr, nullptr, 0), TO_ERR_ARGUMENT, "Nref must be >= 1", "Nref < 1");
  refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, nullptr, 2), TO_ERR_ARGUMENT, "end_mode must be", "unknown end_mode");
  refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, nullptr, -1), TO_ERR_ARGUMENT, "end_mode must be", "unknown end_mode");
  {
    std::vector<double> Xb = X;
    Xb[2 + (size_t)n * (5 + (size_t)Nref * 1)] = nan;  // trajectory 1, knot 6 — and a later one that must not be the one named
    Xb[0 + (size_t)n * (0 + (size_t)Nref * 2)] = inf;
    refusal(validate_tracking_reference(f, Nref, Xb.data(), U.data(), start.data(), 0), TO_ERR_ARGUMENT, "trajectory 1 is not finite at knot 6", "non-finite x");
    std::vector<double> Ub = U;
    Ub[0 + (size_t)m * (7 + (size_t)Nref * 0)] = -inf;
    refusal(validate_tracking_reference(f, Nref, X.data(), Ub.data(), start.data(), 0), TO_ERR_ARGUMENT, "trajectory 0 is not finite at knot 8", "non-finite u");
  }
  {
    std::vector<int32_t> s = {1, 0, 1};
    refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, s.data(), TO_TRACK_END_REFUSE), TO_ERR_ARGUMENT, "start of trajectory 1 is 0", "start < 1");
    refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, s.data(), TO_TRACK_END_HOLD), TO_ERR_ARGUMENT, "start of trajectory 1 is 0", "start < 1, hold");
    s = {1, 1, 5};  // 5 - 1 + 5 = 9 > 8
    refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, s.data(), TO_TRACK_END_REFUSE), TO_ERR_ARGUMENT, "too short for trajectory 2", "window off the end, refuse");
    refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, s.data(), TO_TRACK_END_HOLD), TO_OK, nullptr, "window off the end, hold");
    s = {1, 1, 4};  // 4 - 1 + 5 = 8: the last window that fits
    refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, s.data(), TO_TRACK_END_REFUSE), TO_OK, nullptr, "last window that fits");
    s = {8, 9, 1};
    refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, s.data(), TO_TRACK_END_HOLD), TO_ERR_ARGUMENT, "start of trajectory 1 is 9, behind the reference", "start > Nref, hold");
    s = {8, 8, 1};
    refusal(validate_tracking_reference(f, Nref, X.data(), nullptr, s.data(), TO_TRACK_END_HOLD), TO_OK, nullptr, "start = Nref, hold");
    refusal(validate_tracking_reference(f, N - 1, X.data(), nullptr, nullptr, TO_TRACK_END_REFUSE), TO_ERR_ARGUMENT, "too short for trajectory 0", "Nref < N, refuse");
  }
  {
    std::vector<int> shared = {0, 1, 2, 1, 4};
    TrackFacts g = f;
    g.cost_index = shared.data();
    refusal(validate_tracking_reference(g, Nref, X.data(), nullptr, nullptr, 0), TO_ERR_ARGUMENT, "needs a tracking objective (a distinct cost per knot)", "shared cost");
    g.Nref_set = Nref;
    refusal(validate_tracking_window(g, start.data()), TO_ERR_ARGUMENT, "needs a tracking objective (a distinct cost per knot)", "shared cost, window");
  }
  {
    TrackFacts g = f;
    g.in_flight = true;
    refusal(validate_tracking_reference(g, Nref, X.data(), nullptr, nullptr, 0), TO_ERR_ARGUMENT, "solve is in flight", "in flight");
    g.Nref_set = Nref;
    refusal(validate_tracking_window(g, start.data()), TO_ERR_ARGUMENT, "solve is in flight", "in flight, window");
  }
  // TO_ERR_UNSUPPORTED
  {
    std::vector<to_cost_desc> eq = costs;
    eq[3].kind = TO_COST_ERROR_QUADRATIC;
    TrackFacts g = f;
    g.costs = eq.data();
    refusal(validate_tracking_reference(g, Nref, X.data(), nullptr, nullptr, 0), TO_ERR_UNSUPPORTED, "knot 4 is ErrorQuadratic", "ErrorQuadratic");
    g.Nref_set = Nref;  // a cost replaced by to_set_cost after the reference was stored
    refusal(validate_tracking_window(g, start.data()), TO_ERR_UNSUPPORTED, "knot 4 is ErrorQuadratic", "ErrorQuadratic, window");
    const char* names[5] = {"hybrid double integrator", "model vector", "InfeasibleModel (double integrator, D = 1)", "InfeasibleModel (double integrator, D = 2)",
                            "InfeasibleModel (Cartpole)"};
    for (int key = 7; key <= 11; ++key) {
      TrackFacts u = f;
      u.model_key = key; u.model_name = names[key - 7];
      refusal(validate_tracking_reference(u, Nref, X.data(), nullptr, nullptr, 0), TO_ERR_UNSUPPORTED, names[key - 7], "model");
    }
    for (int key = 0; key <= 6; ++key) {
      TrackFacts u = f;
      u.model_key = key;
      refusal(validate_tracking_reference(u, Nref, X.data(), nullptr, nullptr, 0), TO_OK, nullptr, "model accepted");
    }
  }
  // the window call
  refusal(validate_tracking_window(f, start.data()), TO_ERR_ARGUMENT, "no tracking reference is set", "window without a reference");
  {
    TrackFacts g = f;
    g.Nref_set = Nref; g.end_mode_set = TO_TRACK_END_REFUSE;
    refusal(validate_tracking_window(g, nullptr), TO_ERR_NULL, "start is NULL", "window start NULL");
    refusal(validate_tracking_window(g, start.data()), TO_OK, nullptr, "window accepted");
    std::vector<int32_t> s = {1, 5, 1};
    refusal(validate_tracking_window(g, s.data()), TO_ERR_ARGUMENT, "too short for trajectory 1", "window off the end, refuse");
    g.end_mode_set = TO_TRACK_END_HOLD;
    refusal(validate_tracking_window(g, s.data()), TO_OK, nullptr, "window off the end, hold");
    s = {1, 5, 9};
    refusal(validate_tracking_window(g, s.data()), TO_ERR_ARGUMENT, "start of trajectory 2 is 9", "window start > Nref, hold");
    s = {-2, 5, 8};
    refusal(validate_tracking_window(g, s.data()), TO_ERR_ARGUMENT, "start of trajectory 0 is -2", "window start < 1");
  }
  // the packed upload: rows [x; u] per reference knot, u rows zero without controls
  {
    std::vector<double> Xv((size_t)n * Nref * B), Uv((size_t)m * Nref * B), packed;
    for (auto& v : Xv) v = next_value();
    for (auto& v : Uv) v = next_value();
    for (int with_u = 0; with_u < 2; ++with_u) {
      pack_tracking_reference(n, m, B, Nref, Xv.data(), with_u ? Uv.data() : nullptr, &packed);
      expect(packed.size() == (size_t)(n + m) * Nref * B, "packed size", "");
      for (int b = 0; b < B; ++b)
        for (int j = 0; j < Nref; ++j) {
          for (int i = 0; i < n; ++i) expect(same_bits(packed[i + (size_t)(n + m) * (j + (size_t)Nref * b)], Xv[i + (size_t)n * (j + (size_t)Nref * b)]), "packed x", "");
          for (int i = 0; i < m; ++i)
            expect(same_bits(packed[n + i + (size_t)(n + m) * (j + (size_t)Nref * b)], with_u ? Uv[i + (size_t)m * (j + (size_t)Nref * b)] : 0.0), "packed u", "");
        }
    }
  }
}

int main() {
  const int shapes[4][3] = {{2, 1, 4}, {4, 1, 21}, {13, 4, 15}, {4, 2, 9}};
  const int batches[4] = {1, 64, 65, 130};
  for (int si = 0; si < 4; ++si)
    for (int B : batches) {
      const int n = shapes[si][0], m = shapes[si][1], N = shapes[si][2];
      for (int Nref : {N, N + 7})
        for (int start_mode = 0; start_mode < 3; ++start_mode)
          for (int with_u = 0; with_u < 2; ++with_u)
            for (int wide = 0; wide < 2; ++wide) one_case(n, m, N, B, Nref, start_mode, with_u != 0, si == 3, wide != 0);
    }
  validation_cases();
  std::printf("checks %lld fails %lld\n", g_checks, g_fails);
  return g_fails == 0 ? 0 : 1;
}
