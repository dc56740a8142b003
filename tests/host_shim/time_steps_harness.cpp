// Compiles the host-only lowering of per-trajectory time steps (csrc/desc_lower.h lower_time_steps — what to_set_time_steps_batch runs before
// anything reaches the device) as a program of its own (test infrastructure; tests/test_time_steps_host.py, which also builds it with
// -fsanitize=address,undefined).  Checks the tiling — step k of trajectory b at ((b >> 6) * (N - 1) + k) * 64 + (b & 63), the padding lanes of
// the last tile and the whole spare tile on the SHARED steps, the length DevProblem::dtb is allocated with — and the set -> get round trip
// through the tiled array, and prints
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

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

static void tiling(int N, int B) {
  const int L = N - 1, Bp = (B + 63) / 64 * 64;
  std::vector<double> dt((size_t)L * B), shared(L), tiled(3, -1.0);
  for (int k = 0; k < L; ++k) shared[k] = 0.05 + 1e-3 * k;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < L; ++k) dt[k + (size_t)L * b] = 0.01 * (b + 1) + 1e-4 * (k + 1);   // every entry distinct
  const int rc = lower_time_steps(N, B, Bp, dt.data(), shared.data(), &tiled);
  CHECK(rc == TO_OK, "N %d B %d: rc %d (%s)", N, B, rc, g_err.c_str());
  const size_t tiles = (size_t)Bp / 64 + 1;
  CHECK(tiled.size() == tiles * L * 64 && tiled.size() == time_steps_tiled_len(N, Bp), "N %d B %d: %zu doubles", N, B, tiled.size());
  size_t live = 0;
  for (size_t t = 0; t < tiles; ++t)
    for (int k = 0; k < L; ++k)
      for (int l = 0; l < 64; ++l) {
        const size_t b = t * 64 + l;
        const double v = tiled[(t * L + k) * 64 + l];
        if (b < (size_t)B) { CHECK(v == dt[k + (size_t)L * b], "N %d B %d: step %d of trajectory %zu", N, B, k, b); ++live; }
        else CHECK(v == shared[k], "N %d B %d: padding lane %zu (tile %zu), step %d holds %g, not the shared %g", N, B, b, t, k, v, shared[k]);
      }
  CHECK(live == (size_t)L * B, "N %d B %d: live entries", N, B);
  // the address the kernels form (problem_dev.h dt_lane / step_dt), and the round trip set -> get through it
  std::vector<double> back((size_t)L * B);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < L; ++k) back[k + (size_t)L * b] = tiled[(((size_t)(b >> 6)) * L + k) * 64 + (b & 63)];
  CHECK(back == dt, "N %d B %d: round trip", N, B);
  // the spare tile: where a kernel's idle lanes of trajectory Bp .. Bp + 63 read
  for (int k = 0; k < L; ++k) CHECK(tiled[(((size_t)(Bp >> 6)) * L + k) * 64 + 63] == shared[k], "N %d B %d: spare tile", N, B);
}
static void refusal(const char* name, int N, int B, std::vector<double> dt) {
  std::vector<double> shared(N - 1, 0.1), tiled(2, 7.0);
  g_err.clear();
  const int rc = lower_time_steps(N, B, (B + 63) / 64 * 64, dt.data(), shared.data(), &tiled);
  CHECK(rc != TO_OK ? (tiled.size() == 2 && tiled[0] == 7.0) : true, "%s: the output was touched by a refused call", name);
  printf("case %s code %d msg %s\n", name, rc, g_err.c_str());
}

int main() {
  for (int N : {2, 3, 31, 51})
    for (int B : {1, 6, 63, 64, 65, 70, 128, 300}) tiling(N, B);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int N = 4, B = 3;   // dt[k + 3 b]
  refusal("nan", N, B, {0.1, 0.1, 0.1, 0.1, nan, 0.1, 0.1, 0.1, 0.1});
  refusal("inf", N, B, {0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, inf});
  refusal("zero", N, B, {0.1, 0.1, 0.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1});
  refusal("negative", N, B, {0.1, 0.1, 0.1, 0.1, 0.1, 0.1, -0.2, 0.1, 0.1});
  refusal("first_of_two", N, B, {0.1, 0.1, 0.1, 0.1, 0.1, -1.0, 0.1, nan, 0.1});
  refusal("fine", N, B, {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 1e-300});   // no "must sum to tf - t0" check, no lower limit but > 0
  printf("fails %d\n", fails);
  return fails ? 1 : 0;
}
