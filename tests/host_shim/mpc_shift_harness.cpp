// Compiles csrc/k_mpc.h — the kernels of to_mpc_advance — for the host and runs them thread by thread (test infrastructure;
// tests/test_mpc_advance_host.py builds this as a stand-alone program under AddressSanitizer + UBSan).  Every array has exactly the size
// the entry point gives it, so a row too far is a heap overflow the sanitizer reports; every result is compared, bit for bit, with the
// plain loop   Unew[k] = k + s <= N-2 ? V[k + s] : tail.
// Cases: (n, m, N) in {(2,1,4), (4,1,21), (13,4,15)}, B in {1, 64, 65, 130}, s in {1, 2, N-2}, both guesses, both tails, chunks of one
// wave and of all waves (the staging pair is re-filled per chunk, as the policy kernel does).  Output: "checks <count> fails <count>".
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; };
static dim3 blockIdx, threadIdx, gridDim;
#define __launch_bounds__(x)

#include "k_mpc.h"

using namespace to;

static long long g_checks = 0, g_fails = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
// any bit pattern that is a finite double or a signed zero: equality is checked on bits
static double next_value() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  if ((g_rng & 63) == 0) return (g_rng & 64) ? -0.0 : 0.0;
  uint64_t bits = (g_rng & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 8 + (g_rng >> 52) % 16) << 52);
  double v;
  std::memcpy(&v, &bits, sizeof v);
  return v;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static void expect(bool ok, const char* what, int n, int m, int N, int B, int s, int guess, int tail, int chunk, long long at) {
  ++g_checks;
  if (ok) return;
  if (++g_fails <= 20) std::printf("FAIL %s: n %d m %d N %d B %d s %d guess %d tail %d chunk %d at %lld\n", what, n, m, N, B, s, guess, tail, chunk, at);
}

template <class K, class... A>
static void run(K kernel, unsigned gx, unsigned gy, const A&... args) {
  gridDim.x = gx; gridDim.y = gy;
  for (blockIdx.y = 0; blockIdx.y < gy; ++blockIdx.y)
    for (blockIdx.x = 0; blockIdx.x < gx; ++blockIdx.x)
      for (threadIdx.x = 0; threadIdx.x < 64; ++threadIdx.x) kernel(args...);
}

static std::unique_ptr<double[]> filled(size_t count) {
  std::unique_ptr<double[]> p(new double[count]);
  for (size_t i = 0; i < count; ++i) p[i] = next_value();
  return p;
}

static void one_case(int n, int m, int N, int B, int s, int guess, int tail, int chunk, bool wide) {
  const int tiles = (B + 63) / 64, Lx = N * n, Lu = (N - 1) * m;
  const size_t nx0 = (size_t)tiles * n * 64, nus = (size_t)tiles * Lu * 64;
  // what the policy kernel computes for every lane of every tile (lanes behind the batch roll out a copy: values that must go nowhere)
  auto Xcl = filled((size_t)tiles * Lx * 64), Ucl = filled((size_t)tiles * Lu * 64);
  auto x0 = filled(nx0), Us = filled(nus);
  std::unique_ptr<int[]> status(new int[B]);
  for (int b = 0; b < B; ++b) status[b] = (b % 5 == 3 || (B > 1 && b == B - 1)) ? 6 + (b & 1) : 0;
  std::vector<double> x0_old(x0.get(), x0.get() + nx0), Us_old(Us.get(), Us.get() + nus);
  const size_t cx = (size_t)n * B, cX = (size_t)n * (s + 1) * B, cU = (size_t)m * s * B;
  auto x_next = filled(cx), X_applied = filled(cX), U_applied = filled(cU);
  std::unique_ptr<double[]> Xw(new double[(size_t)chunk * Lx * 64]), Uw(new double[(size_t)chunk * Lu * 64]);
  MpcArgs a;
  std::memset(&a, 0, sizeof a);
  a.n = n; a.m = m; a.N = N; a.B = B; a.s = s; a.guess = guess; a.tail = tail;
  double fill[MPC_MAX_M];
  for (int j = 0; j < MPC_MAX_M; ++j) a.u_fill[j] = fill[j] = next_value();
  a.Xw = Xw.get(); a.Uw = Uw.get(); a.status = status.get(); a.x0 = x0.get(); a.Us = Us.get();
  a.x_next = x_next.get(); a.X_applied = X_applied.get(); a.U_applied = U_applied.get();
  const int rows = Lu > (s + 1) * n ? Lu : (s + 1) * n;
  auto advance = [&] {  // the chunk loop of the entry point; the two memcpy stand for the policy kernel of the chunk
    for (int g0 = 0; g0 < tiles; g0 += chunk) {
      const int ng = chunk < tiles - g0 ? chunk : tiles - g0;
      std::memcpy(Xw.get(), Xcl.get() + (size_t)g0 * Lx * 64, sizeof(double) * (size_t)ng * Lx * 64);
      std::memcpy(Uw.get(), Ucl.get() + (size_t)g0 * Lu * 64, sizeof(double) * (size_t)ng * Lu * 64);
      a.g0 = g0;
      run(k_mpc_writeback, (unsigned)ng, (unsigned)(!wide ? 1 : (rows < 32 ? rows : 32)), a);
      if (guess == 1) run(k_mpc_shift_nominal, (unsigned)ng, 1u, a);
    }
  };
  advance();
  auto tiled = [](const double* p, int L, int b, int e) { return p[((size_t)(b >> 6) * L + e) * 64 + (b & 63)]; };
  for (int b = 0; b < tiles * 64; ++b) {
    const bool moved = b < B && status[b] == 0;
    for (int i = 0; i < n; ++i) {
      const double want = moved ? tiled(Xcl.get(), Lx, b, s * n + i) : tiled(x0_old.data(), n, b, i);
      expect(same_bits(tiled(x0.get(), n, b, i), want), moved ? "x0" : "x0 kept", n, m, N, B, s, guess, tail, chunk, (long long)b * n + i);
    }
    for (int k = 0; k < N - 1; ++k)
      for (int j = 0; j < m; ++j) {
        const double* V = guess == 0 ? Ucl.get() : Us_old.data();
        double want = tiled(Us_old.data(), Lu, b, k * m + j);
        if (moved) want = k + s <= N - 2 ? tiled(V, Lu, b, (k + s) * m + j) : tail == 0 ? tiled(V, Lu, b, (N - 2) * m + j) : fill[j];
        expect(same_bits(tiled(Us.get(), Lu, b, k * m + j), want), moved ? "U" : "U kept", n, m, N, B, s, guess, tail, chunk, ((long long)b * (N - 1) + k) * m + j);
      }
    if (b >= B) continue;
    for (int i = 0; i < n; ++i)
      expect(same_bits(x_next[(size_t)i + (size_t)n * b], tiled(Xcl.get(), Lx, b, s * n + i)), "x_next", n, m, N, B, s, guess, tail, chunk, (long long)b * n + i);
    for (int k = 0; k <= s; ++k)
      for (int i = 0; i < n; ++i)
        expect(same_bits(X_applied[(size_t)i + (size_t)n * (k + (size_t)(s + 1) * b)], tiled(Xcl.get(), Lx, b, k * n + i)), "X_applied", n, m, N, B, s, guess, tail, chunk, k);
    for (int k = 0; k < s; ++k)
      for (int j = 0; j < m; ++j)
        expect(same_bits(U_applied[(size_t)j + (size_t)m * (k + (size_t)s * b)], tiled(Ucl.get(), Lu, b, k * m + j)), "U_applied", n, m, N, B, s, guess, tail, chunk, k);
  }
  {  // a caller that wants none of the host arrays: the three gathers off, the same writes
    std::vector<double> x0_new(x0.get(), x0.get() + nx0), Us_new(Us.get(), Us.get() + nus);
    std::memcpy(x0.get(), x0_old.data(), sizeof(double) * nx0);
    std::memcpy(Us.get(), Us_old.data(), sizeof(double) * nus);
    a.x_next = a.X_applied = a.U_applied = nullptr;
    advance();
    expect(std::memcmp(x0.get(), x0_new.data(), sizeof(double) * nx0) == 0, "x0 without gathers", n, m, N, B, s, guess, tail, chunk, 0);
    expect(std::memcmp(Us.get(), Us_new.data(), sizeof(double) * nus) == 0, "U without gathers", n, m, N, B, s, guess, tail, chunk, 0);
  }
  // the start states when no measurement is given: tiled x0 -> [n, B]
  std::unique_ptr<double[]> x0s(new double[cx]);
  run(k_mpc_x0_in, (unsigned)tiles, 1u, (const double*)x0.get(), x0s.get(), n, B);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < n; ++i) expect(same_bits(x0s[(size_t)b * n + i], tiled(x0.get(), n, b, i)), "x0_in", n, m, N, B, s, guess, tail, chunk, (long long)b * n + i);
}

int main() {
  const int shapes[3][3] = {{2, 1, 4}, {4, 1, 21}, {13, 4, 15}};
  const int batches[4] = {1, 64, 65, 130};
  for (const auto& sh : shapes)
    for (int B : batches) {
      const int n = sh[0], m = sh[1], N = sh[2], tiles = (B + 63) / 64;
      const int shifts[3] = {1, 2, N - 2};
      for (int si = 0; si < 3; ++si) {
        if (si == 2 && (N - 2 == 1 || N - 2 == 2)) continue;  // (N = 4: N-2 = 2 is there already)
        for (int guess = 0; guess < 2; ++guess)
          for (int tail = 0; tail < 2; ++tail)
            for (int all = 0; all < 2; ++all)  // chunks of one wave with one row group, all waves in one chunk with up to 32 row groups
              one_case(n, m, N, B, shifts[si], guess, tail, all ? tiles : 1, all != 0);
      }
    }
  std::printf("checks %lld fails %lld\n", g_checks, g_fails);
  return g_fails == 0 ? 0 : 1;
}
