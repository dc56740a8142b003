// Compiles csrc/k_mpc.h — here the kernel of to_mpc_shift_duals — for the host and runs it thread by thread (test infrastructure;
// tests/test_mpc_dual_shift_host.py builds this as a stand-alone program with and without AddressSanitizer + UBSan).  The dual and penalty
// arrays have exactly the size the handle gives them (n_duals x Bp and n_cons x Bp doubles), so a row too far is a heap overflow the
// sanitizer reports; every element is compared, bit for bit, with the scalar restatement
//     SHIFT: new[r, j] = j + s < nk ? old[r, j + s] : (hold ? old[r, nk - 1] : 0)      RESET: new = 0, mu = mu_reset      LEAVE: unchanged
// and everything the semantics do not name — the padding lanes behind B, the penalties of trajectories that are not reset — keeps the random
// pattern it was filled with.
// Cases: B in {1, 64, 70, 130}; constraint tables  {p=6 nk=10, p=4 nk=5, p=1 nk=1}, {p=1 nk=7}, {p=4 nk=1, p=6 nk=3}  (knot ranges that start
// at 0 and above 0 differ only in nk and dual_off here: the kernel never sees k1); s in {1, 2, 4, nk_max - 1, nk_max, nk_max + 3}; both tails; actions
// NULL, all LEAVE, all SHIFT, all RESET and a seeded mix.  Then the host-only refusals of csrc/desc_lower.h validate_mpc_shift_duals.
// Output: "checks <count> fails <count>".
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; };
static dim3 blockIdx, threadIdx, gridDim;
#define __launch_bounds__(x)

#include "k_mpc.h"
#include "desc_lower.h"

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

static long long g_checks = 0, g_fails = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t next_bits() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
// any bit pattern that is a finite double or a signed zero: equality is checked on bits
static double next_value() {
  const uint64_t r = next_bits();
  if ((r & 63) == 0) return (r & 64) ? -0.0 : 0.0;
  uint64_t bits = (r & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 8 + (r >> 52) % 16) << 52);
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

static void run(const MpcDualArgs& a, unsigned gx, unsigned gy) {
  gridDim.x = gx; gridDim.y = gy;
  for (blockIdx.y = 0; blockIdx.y < gy; ++blockIdx.y)
    for (blockIdx.x = 0; blockIdx.x < gx; ++blockIdx.x)
      for (threadIdx.x = 0; threadIdx.x < 64; ++threadIdx.x) k_mpc_shift_duals(a);
}

struct Con { int p, k1, k2; };

static void one_case(const std::vector<Con>& cons, int B, int s, int tail, int mix) {
  const int tiles = (B + 63) / 64, Bp = tiles * 64, nc = (int)cons.size();
  std::vector<MpcDualCon> table;
  long long n_duals = 0;
  for (const Con& c : cons) { table.push_back(MpcDualCon{n_duals, c.p, c.k2 - c.k1 + 1}); n_duals += (long long)c.p * (c.k2 - c.k1 + 1); }
  // exactly the handle's sizes, on the heap
  std::vector<double> lam((size_t)n_duals * Bp), mu((size_t)nc * Bp);
  for (double& v : lam) v = next_value();
  for (double& v : mu) v = next_value();
  const std::vector<double> lam_old = lam, mu_old = mu;
  std::vector<int> action(B);  // exactly B entries: a lane behind the batch that read its action would read past the end
  for (int b = 0; b < B; ++b) action[b] = mix == 1 ? 0 : mix == 2 ? 1 : mix == 3 ? 2 : (int)(next_bits() % 3);
  const double mu_reset = next_value();
  MpcDualArgs a;
  std::memset(&a, 0, sizeof a);
  a.B = B; a.n_cons = nc; a.s = s; a.tail = tail; a.n_duals = n_duals; a.mu_reset = mu_reset;
  a.cons = table.data(); a.action = mix == 0 ? nullptr : action.data(); a.lam = lam.data(); a.mu = mu.data();
  run(a, (unsigned)tiles, (unsigned)nc);
  const std::string tag = "B " + std::to_string(B) + " s " + std::to_string(s) + " tail " + std::to_string(tail) + " mix " + std::to_string(mix) + " cons " + std::to_string(nc);
  auto at = [&](const std::vector<double>& v, long long L, int b, long long e) { return v[((size_t)(b >> 6) * L + e) * 64 + (b & 63)]; };
  for (int b = 0; b < Bp; ++b) {
    const int act = b >= B ? 0 : (mix == 0 ? 1 : action[b]);
    for (int ci = 0; ci < nc; ++ci) {
      const int p = table[ci].p, nk = table[ci].nk;
      for (int j = 0; j < nk; ++j)
        for (int r = 0; r < p; ++r) {
          const long long e = table[ci].dual_off + (long long)j * p + r;
          double want = at(lam_old, n_duals, b, e);
          if (act == 1) want = j + s < nk ? at(lam_old, n_duals, b, table[ci].dual_off + (long long)(j + s) * p + r)
                                          : tail == 0 ? at(lam_old, n_duals, b, table[ci].dual_off + (long long)(nk - 1) * p + r) : 0.0;
          if (act == 2) want = 0.0;
          expect(same_bits(at(lam, n_duals, b, e), want), b >= B ? "padding lane" : act == 0 ? "lambda left" : act == 1 ? "lambda shifted" : "lambda reset",
                 tag + " b " + std::to_string(b) + " con " + std::to_string(ci) + " knot " + std::to_string(j) + " row " + std::to_string(r));
        }
      expect(same_bits(at(mu, nc, b, ci), act == 2 ? mu_reset : at(mu_old, nc, b, ci)), act == 2 ? "mu reset" : "mu kept", tag + " b " + std::to_string(b) + " con " + std::to_string(ci));
    }
  }
}

static void refusals() {
  const int N = 11, B = 5;
  auto facts = [&](int key, bool busy) { return MpcDualFacts{key, "NamedModel", N, B, busy}; };
  std::vector<int32_t> act(B, TO_MPC_DUAL_SHIFT);
  expect(validate_mpc_shift_duals(facts(0, false), 1, TO_MPC_DUAL_TAIL_HOLD, nullptr) == TO_OK, "accepts", "NULL action");
  expect(validate_mpc_shift_duals(facts(6, false), N - 2, TO_MPC_DUAL_TAIL_ZERO, act.data()) == TO_OK, "accepts", "s = N-2, key 6");
  act[2] = TO_MPC_DUAL_RESET; act[3] = TO_MPC_DUAL_LEAVE;
  expect(validate_mpc_shift_duals(facts(3, false), 4, TO_MPC_DUAL_TAIL_HOLD, act.data()) == TO_OK, "accepts", "mixed actions");
  expect(validate_mpc_shift_duals(facts(0, true), 1, 0, nullptr) == TO_ERR_ARGUMENT && g_err.find("in flight") != std::string::npos, "refuses", "solve in flight");
  expect(validate_mpc_shift_duals(facts(7, true), 0, 9, nullptr) == TO_ERR_ARGUMENT && g_err.find("in flight") != std::string::npos, "refuses", "in flight comes first");
  for (int key = 7; key <= 11; ++key)
    expect(validate_mpc_shift_duals(facts(key, false), 1, 0, nullptr) == TO_ERR_UNSUPPORTED && g_err.find("to_mpc_shift_duals: not available for the NamedModel") == 0 &&
               g_err.find("cannot shift their plan") != std::string::npos, "refuses", "model key " + std::to_string(key));
  for (int s : {0, -1, N - 1, N, 1 << 30})
    expect(validate_mpc_shift_duals(facts(0, false), s, 0, nullptr) == TO_ERR_ARGUMENT && g_err.find("shift must be in 1 .. N-2 = 9") != std::string::npos, "refuses", "shift " + std::to_string(s));
  for (int t : {-1, 2, 7})
    expect(validate_mpc_shift_duals(facts(0, false), 1, t, nullptr) == TO_ERR_ARGUMENT && g_err.find("tail must be") != std::string::npos, "refuses", "tail " + std::to_string(t));
  for (int bad : {-1, 3, 100}) {
    std::vector<int32_t> a2(B, TO_MPC_DUAL_SHIFT);
    a2[B - 1] = bad;
    expect(validate_mpc_shift_duals(facts(0, false), 1, 0, a2.data()) == TO_ERR_ARGUMENT && g_err.find("action of trajectory 4 is " + std::to_string(bad)) != std::string::npos,
           "refuses", "action " + std::to_string(bad));
  }
}

int main() {
  const std::vector<std::vector<Con>> tables = {
      {{6, 1, 10}, {4, 4, 8}, {1, 10, 10}},   // the handle of the GPU test: bounds on knots 1..N-1, bounds on 4..8, a terminal row
      {{1, 0, 6}},
      {{4, 0, 0}, {6, 2, 4}},
  };
  const int batches[4] = {1, 64, 70, 130};
  for (const auto& cons : tables) {
    int nk_max = 0;
    for (const Con& c : cons) nk_max = c.k2 - c.k1 + 1 > nk_max ? c.k2 - c.k1 + 1 : nk_max;
    std::vector<int> shifts = {1, 2, 4, nk_max - 1, nk_max, nk_max + 3};  // (2 and 4: nk - 1 of the shorter ranges)
    for (int B : batches)
      for (int s : shifts) {
        if (s < 1) continue;
        for (int tail = 0; tail < 2; ++tail)
          for (int mix = 0; mix < 5; ++mix) one_case(cons, B, s, tail, mix);
      }
  }
  refusals();
  std::printf("checks %lld fails %lld\n", g_checks, g_fails);
  return g_fails == 0 ? 0 : 1;
}
