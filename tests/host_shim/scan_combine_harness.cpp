// Compiles csrc/scan_combine.h for the host (test infrastructure; tests/test_scan_combine_host.py, which also builds it with
// -fsanitize=address,undefined).  Checks, on bytes (memcmp: -0.0 != +0.0):
//   1. the value-only form of scan_combine gives the (eta, J) of the full form, over seeded random elements (A general, C and J
//      positive semidefinite) and over chains of combinations, n = 2 and n = 4;
//   2. combine(identity, identity) is the identity;
//   3. a 64-lane suffix scan simulated lane by lane: the trimmed round loop of k_scan.h (full rounds, then a value-only last round, the
//      clamped read of lane 63 taken as it is) against the untrimmed one (every round full, the neutral element selected past lane 63):
//      the same (J, eta) in every lane, for every block count 1..63, and lane 63 the identity after every round.
#include <hip/hip_runtime.h>
#include "scan_combine.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
using namespace to;

static long long fails = 0, checks = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

template <int n>
static void psd(std::mt19937_64& rng, double* packed, int rank) {  // packed upper triangle (ScanEl::sy) of G G', G n x rank
  std::normal_distribution<double> nd;
  double G[n][n] = {};
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < rank; ++j) G[i][j] = nd(rng);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i <= j; ++i) {
      double v = 0.0;
      for (int t = 0; t < rank; ++t) v += G[i][t] * G[j][t];
      packed[ScanEl<n>::sy(i, j)] = v;
    }
}

template <int n>
static ScanEl<n> random_element(std::mt19937_64& rng, int trial) {
  std::normal_distribution<double> nd;
  ScanEl<n> e;
  for (int i = 0; i < n * n; ++i) e.A[i] = nd(rng);
  for (int i = 0; i < n; ++i) { e.b[i] = nd(rng); e.eta[i] = nd(rng); }
  psd<n>(rng, e.C, trial % (n + 1));       // rank 0 (C = 0: a terminal knot) .. n
  psd<n>(rng, e.J, (trial / (n + 1)) % (n + 1));
  if (trial % 7 == 3) for (int i = 0; i < n * n; ++i) e.A[i] = 0.0;  // the terminal knot's element: (0, 0, 0, q, Q)
  return e;
}

template <int n>
static bool same_value(const ScanEl<n>& a, const ScanEl<n>& b) {
  return std::memcmp(a.eta, b.eta, sizeof(a.eta)) == 0 && std::memcmp(a.J, b.J, sizeof(a.J)) == 0;
}
template <int n>
static bool same_bytes(const ScanEl<n>& a, const ScanEl<n>& b) {
  return same_value(a, b) && std::memcmp(a.A, b.A, sizeof(a.A)) == 0 && std::memcmp(a.b, b.b, sizeof(a.b)) == 0 && std::memcmp(a.C, b.C, sizeof(a.C)) == 0;
}

template <int n>
static void value_only_matches(unsigned seed) {
  std::mt19937_64 rng(seed);
  for (int trial = 0; trial < 2000; ++trial) {
    ScanEl<n> e1 = random_element<n>(rng, trial), e2 = random_element<n>(rng, trial / 3 + 1);
    for (int depth = 0; depth < 4; ++depth) {  // and on elements that are combinations themselves
      ScanEl<n> full, val;
      std::memset(&val, 0xff, sizeof(val));
      scan_combine<n>(e1, e2, full);
      ScanEl<n> e2v = e2;  // the value-only form must not read A, b, C of the later span: poison them
      std::memset(e2v.A, 0xff, sizeof(e2v.A)); std::memset(e2v.b, 0xff, sizeof(e2v.b)); std::memset(e2v.C, 0xff, sizeof(e2v.C));
      scan_combine<n, true>(e1, e2v, val);
      CHECK(same_value(full, val), "n %d trial %d depth %d: value-only (eta, J) differ from the full form", n, trial, depth);
      unsigned char ff[sizeof(val.A)];
      std::memset(ff, 0xff, sizeof(ff));
      CHECK(std::memcmp(val.A, ff, sizeof(val.A)) == 0 && std::memcmp(val.b, ff, sizeof(val.b)) == 0 && std::memcmp(val.C, ff, sizeof(val.C)) == 0,
            "n %d: the value-only form wrote A, b or C", n);
      e2 = full;
      e1 = random_element<n>(rng, trial + depth);
    }
  }
}

template <int n>
static void identity_is_neutral_on_itself() {
  ScanEl<n> id, o;
  id.identity();
  scan_combine<n>(id, id, o);
  CHECK(same_bytes(id, o), "n %d: combine(identity, identity) is not the identity's bytes", n);
  ScanEl<n> v;
  v.identity();
  scan_combine<n, true>(id, id, v);
  CHECK(same_bytes(id, v), "n %d: value-only combine(identity, identity)", n);
}

// the round loops of k_expand_backward_scan on a simulated wave
template <int n>
static void wave_scan(unsigned seed) {
  std::mt19937_64 rng(seed);
  ScanEl<n> id;
  id.identity();
  for (int NB = 1; NB <= 63; ++NB) {
    std::vector<ScanEl<n>> a(64), t(64), nx(64);
    for (int l = 0; l < 64; ++l) a[l] = t[l] = (l < NB) ? random_element<n>(rng, l + NB) : id;
    for (int d = 1; d < NB; d <<= 1) {  // untrimmed: every round full, the neutral element selected past lane 63
      for (int l = 0; l < 64; ++l) {
        const ScanEl<n> pe = (l + d < 64) ? a[l + d] : id;
        scan_combine<n>(a[l], pe, nx[l]);
      }
      a = nx;
    }
    int d = 1;
    for (; 2 * d < NB; d <<= 1) {       // trimmed: full rounds with the clamped read as it is ...
      for (int l = 0; l < 64; ++l) scan_combine<n>(t[l], t[l + d < 64 ? l + d : 63], nx[l]);
      t = nx;
      CHECK(same_bytes(t[63], id), "n %d NB %d d %d: lane 63 left the identity", n, NB, d);
    }
    if (d < NB) {                       // ... then the value part of the last round
      for (int l = 0; l < 64; ++l) {
        nx[l] = t[l];
        scan_combine<n, true>(t[l], t[l + d < 64 ? l + d : 63], nx[l]);
      }
      t = nx;
    }
    for (int l = 0; l < 64; ++l) CHECK(same_value(a[l], t[l]), "n %d NB %d lane %d: trimmed scan (J, eta) differ", n, NB, l);
  }
}

int main() {
  value_only_matches<2>(11);
  value_only_matches<4>(12);
  identity_is_neutral_on_itself<2>();
  identity_is_neutral_on_itself<4>();
  wave_scan<2>(21);
  wave_scan<4>(22);
  printf("checks %lld fails %lld\n", checks, fails);
  return fails ? 1 : 0;
}
