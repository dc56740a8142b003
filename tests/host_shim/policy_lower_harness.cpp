// Compiles the host-only lowering of the closed-loop rollouts and the receding-horizon step (csrc/policy_lower.h: lower_policy_opts — what
// to_policy_rollout, to_policy_rollout_mc and to_mpc_advance run before their first device call — and lower_mpc_opts) as a program of its own
// (test infrastructure; tests/test_policy_lower_host.py, which also builds it with -fsanitize=address,undefined).  Prints
//   case <name> code <c> msg <text> : every refusal, with the error class and the message,
// and checks what an accepted call fills: the kernel's NZ, the per-sample plants of a handle with its own, the clamp, the lane map, the
// refusal of a call with too many waves (only the plan is computed: nothing is allocated), MpcArgs::u_fill.  Ends with  fails <n>.
#include <hip/hip_runtime.h>

#include "policy_lower.h"

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
static const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();

// a quaternion Quadrotor handle, B = 3, every instance compiled
static double g_mp[16];
static PolicyFacts quad() {
  for (int i = 0; i < 16; ++i) g_mp[i] = 0.5 + i;
  g_mp[10] = TO_ROT_QUATERNION;
  return PolicyFacts{4, g_mp, 13, 4, 12, 11, 3, false, false, nullptr, true, true, 7, 0, nullptr, nullptr};
}
static const to_policy_opts kDefault = {1, 0, 0.0, nullptr, nullptr, nullptr};
struct Out { int rc; PolicyRun run; const double* plants; };
static const double kSentinel = 7.0;
static Out lower(const char* name, const PolicyFacts& f, int S, const to_policy_opts* o, const to_policy_noise* nz, bool force_packed = false) {
  Out out;
  std::memset(&out.run.pa, 0, sizeof(out.run.pa));
  out.run.waves = -7; out.run.own_plants.assign(2, kSentinel);
  out.plants = &kSentinel;
  g_err.clear();
  out.rc = lower_policy_opts(f, S, o, nz, force_packed, &out.run, &out.plants);
  if (out.rc != TO_OK)
    CHECK(out.run.waves == -7 && out.run.own_plants == std::vector<double>(2, kSentinel) && out.plants == &kSentinel, "%s: the output was touched by a refused call", name);
  if (name) printf("case %s code %d msg %s\n", name, out.rc, out.rc == TO_OK ? "" : g_err.c_str());
  return out;
}
static to_policy_noise noise_of(const double* sw, const double* sv, const double* plants) {
  to_policy_noise z;
  std::memset(&z, 0, sizeof(z));
  z.seed = 0x1234567890abcdefull; z.traj_offset = 5; z.sample_offset = 9; z.sigma_w = sw; z.sigma_v = sv; z.plant_params = plants;
  return z;
}

static void policy_refusals() {
  const PolicyFacts f = quad();
  std::vector<double> sigma(12, 0.01), plant(g_mp, g_mp + 16);
  lower("samples", f, 0, nullptr, nullptr);
  { PolicyFacts g = f; g.rollout_compiled = false; lower("not_compiled", g, 2, nullptr, nullptr); }
  { to_policy_opts o = kDefault; o.refresh_gains = 2; lower("refresh_gains", f, 2, &o, nullptr); }
  { to_policy_opts o = kDefault; o.alpha = Inf; lower("alpha", f, 2, &o, nullptr); }
  { std::vector<double> p = plant; p[10] = TO_ROT_MRP; to_policy_opts o = kDefault; o.plant_params = p.data(); lower("plant", f, 2, &o, nullptr); }
  { PolicyFacts g = f; g.model_key = 8; to_policy_opts o = kDefault; o.plant_params = plant.data(); lower("plant_model_vector", g, 2, &o, nullptr); }
  for (int key : {7, 8}) { PolicyFacts g = f; g.model_key = key; to_policy_noise z = noise_of(nullptr, sigma.data(), nullptr); lower(key == 7 ? "sigma_hybrid" : "sigma_model_vector", g, 2, nullptr, &z); }
  { std::vector<double> s = sigma; s[11] = -1e-3; to_policy_noise z = noise_of(s.data(), nullptr, nullptr); lower("sigma_w", f, 2, nullptr, &z); }
  { std::vector<double> s = sigma; s[0] = NaN; to_policy_noise z = noise_of(sigma.data(), s.data(), nullptr); lower("sigma_v", f, 2, nullptr, &z); }
  const int S = 4, B = 3;
  std::vector<double> per_sample((size_t)16 * S * B);
  for (int c = 0; c < S * B; ++c) std::memcpy(&per_sample[(size_t)16 * c], g_mp, sizeof(g_mp));
  {
    to_policy_opts o = kDefault; o.plant_params = plant.data();
    to_policy_noise z = noise_of(nullptr, nullptr, per_sample.data());
    lower("both_plants", f, S, &o, &z);
  }
  {  // the first offending (b, s), behind good ones and ahead of another bad one
    std::vector<double> p = per_sample;
    p[((size_t)1 * S + 2) * 16 + 10] = TO_ROT_RODRIGUES; p[((size_t)2 * S + 0) * 16 + 10] = TO_ROT_MRP;
    to_policy_noise z = noise_of(nullptr, nullptr, p.data());
    lower("order_first_bad_sample", f, S, nullptr, &z);
  }
  { PolicyFacts g = f; g.mc_compiled = false; to_policy_noise z = noise_of(sigma.data(), nullptr, nullptr); lower("mc_not_compiled", g, 2, nullptr, &z); }
  { PolicyFacts g = f; g.noise_mask = 3; to_policy_noise z = noise_of(nullptr, nullptr, per_sample.data()); lower("mc_not_in_mask", g, S, nullptr, &z); }
  {  // a handle with its own plants asks for the one-plant-per-sample instance too
    PolicyFacts g = f; g.noise_mask = 3; g.pm = true; std::vector<double> own((size_t)16 * B, 1.0); g.pm_host = own.data();
    lower("mc_own_plants_not_in_mask", g, 2, nullptr, nullptr);
  }
  const double lo[4] = {-1.0, -1.0, 0.5, -1.0}, hi[4] = {1.0, 1.0, 0.25, 1.0};
  { to_policy_opts o = kDefault; o.u_min = lo; o.u_max = hi; lower("clamp", f, 2, &o, nullptr); }
  { const double nan_hi[4] = {1.0, NaN, 1.0, 1.0}; to_policy_opts o = kDefault; o.u_max = nan_hi; lower("clamp_nan", f, 2, &o, nullptr); }
  { to_policy_opts o = kDefault; o.alpha = NaN; o.u_min = lo; o.u_max = hi; lower("order_alpha_before_clamp", f, 2, &o, nullptr); }
  { to_policy_opts o = kDefault; o.refresh_gains = -1; lower("order_samples_before_refresh", f, -3, &o, nullptr); }
  // too many waves for one call: the limit is 0x7fffffff / 64 = 33 554 431 waves.  Uniform map at S = 65 (2 waves per trajectory): the smallest
  // batch that crosses it is 16 777 216; packed at S = 1 (64 trajectories per wave): 64 * 33 554 431 + 1.  pm is unset: nothing is allocated.
  { PolicyFacts g = f; g.B = 16777216; lower("too_large_uniform", g, 65, nullptr, nullptr); }
  { PolicyFacts g = f; g.B = 16777215; const Out o = lower("largest_uniform", g, 65, nullptr, nullptr); CHECK(o.rc == TO_OK && o.run.waves == 33554430 && o.run.SB == (size_t)65 * 16777215, "waves %d", o.run.waves); }
  { PolicyFacts g = f; g.B = 2147483585; lower("too_large_packed", g, 1, nullptr, nullptr, true); }
  { PolicyFacts g = f; g.B = 2147483584; const Out o = lower("largest_packed", g, 1, nullptr, nullptr, true); CHECK(o.rc == TO_OK && o.run.waves == 33554431, "waves %d", o.run.waves); }
}

static void policy_outputs() {
  const PolicyFacts f = quad();
  const int B = 3;
  std::vector<double> sw(12), sv(12);
  for (int i = 0; i < 12; ++i) { sw[i] = 0.01 * (i + 1); sv[i] = 0.002 * (i + 1); }
  {  // nothing set: to_policy_rollout itself
    const Out o = lower(nullptr, f, 2, nullptr, nullptr);
    CHECK(o.rc == TO_OK && o.run.nz == 0 && o.plants == nullptr && o.run.own_plants.empty() && o.run.refresh_gains, "defaults: nz %d", o.run.nz);
    const PolicyArgs& pa = o.run.pa;
    CHECK(pa.S == 2 && pa.TPW == 32 && pa.WPT == 1 && pa.g0 == 0 && pa.store == 0 && pa.clamp == 0 && pa.alpha == 0.0, "defaults: argument block");
    for (int j = 0; j < TO_MAX_M; ++j) CHECK(pa.u_min[j] == -HUGE_VAL && pa.u_max[j] == HUGE_VAL, "defaults: clamp[%d]", j);
    CHECK(std::memcmp(pa.mp, g_mp, sizeof(g_mp)) == 0, "defaults: the problem's plant");
    CHECK(!pa.x0s && !pa.J && !pa.cmax && !pa.dxmax && !pa.status && !pa.klim && !pa.Xw && !pa.Uw && !pa.plants, "defaults: device pointers are null");
    const PolicyPlan want = plan_policy(13, 4, 11, B, 2, nullptr, nullptr, 0);
    CHECK(o.run.packed && o.run.waves == (int)want.waves && o.run.SB == 6 && o.run.plan.x0s_len == want.x0s_len && o.run.plan.chunk == want.chunk, "defaults: plan");
  }
  // the kernel's NZ
  std::vector<double> per_sample((size_t)16 * 2 * B);
  for (int c = 0; c < 2 * B; ++c) { std::memcpy(&per_sample[(size_t)16 * c], g_mp, sizeof(g_mp)); per_sample[(size_t)16 * c + 3] = 100.0 + c; }
  {
    to_policy_noise z = noise_of(sw.data(), nullptr, nullptr);
    const Out o = lower(nullptr, f, 2, nullptr, &z);
    CHECK(o.rc == TO_OK && o.run.nz == 1 && o.plants == nullptr, "sigma_w only: nz %d", o.run.nz);
    for (int i = 0; i < TO_MAX_N; ++i) CHECK(o.run.pa.sigma_w[i] == (i < 12 ? sw[i] : 0.0) && o.run.pa.sigma_v[i] == 0.0, "sigma_w only: [%d]", i);
    CHECK(o.run.pa.seed == 0x1234567890abcdefull && o.run.pa.traj_offset == 5 && o.run.pa.sample_offset == 9, "counters");
  }
  { to_policy_noise z = noise_of(nullptr, sv.data(), nullptr); const Out o = lower(nullptr, f, 2, nullptr, &z); CHECK(o.rc == TO_OK && o.run.nz == 2 && o.run.pa.sigma_v[11] == sv[11] && o.run.pa.sigma_w[0] == 0.0, "sigma_v only: nz %d", o.run.nz); }
  { to_policy_noise z = noise_of(nullptr, nullptr, per_sample.data()); const Out o = lower(nullptr, f, 2, nullptr, &z); CHECK(o.rc == TO_OK && o.run.nz == 4 && o.plants == per_sample.data() && o.run.own_plants.empty(), "plants only: nz %d", o.run.nz); }
  { to_policy_noise z = noise_of(sw.data(), sv.data(), per_sample.data()); const Out o = lower(nullptr, f, 2, nullptr, &z); CHECK(o.rc == TO_OK && o.run.nz == 7 && o.plants == per_sample.data(), "all three: nz %d", o.run.nz); }
  { to_policy_noise z = noise_of(nullptr, nullptr, nullptr); const Out o = lower(nullptr, f, 2, nullptr, &z); CHECK(o.rc == TO_OK && o.run.nz == 0 && o.run.pa.seed == z.seed, "empty noise: nz %d", o.run.nz); }
  // the handle's own plants, per sample
  std::vector<double> own((size_t)16 * B);
  for (int b = 0; b < B; ++b) { std::memcpy(&own[(size_t)16 * b], g_mp, sizeof(g_mp)); own[(size_t)16 * b + 0] = 10.0 + b; }
  std::vector<double> other(g_mp, g_mp + 16);
  other[0] = 99.0;
  const int S = 2;
  {
    PolicyFacts g = f; g.pm = true; g.pm_host = own.data();
    const Out o = lower(nullptr, g, S, nullptr, nullptr);
    CHECK(o.rc == TO_OK && o.run.nz == 4 && o.plants == o.run.own_plants.data() && o.run.own_plants.size() == (size_t)16 * S * B && o.run.own_plants.size() == o.run.plan.plants_len, "own plants: nz %d", o.run.nz);
    for (int b = 0; b < B && o.run.own_plants.size() == (size_t)16 * S * B; ++b)
      for (int s = 0; s < S; ++s) CHECK(std::memcmp(&o.run.own_plants[((size_t)b * S + s) * 16], &own[(size_t)16 * b], sizeof(double) * 16) == 0, "own plants: (b, s) = (%d, %d)", b, s);
    CHECK(std::memcmp(o.run.pa.mp, g_mp, sizeof(g_mp)) == 0, "own plants: pa.mp is the problem's");
    // an explicit shared plant overrides them: the NZ = 0 kernel on that plant
    to_policy_opts op = kDefault; op.plant_params = other.data();
    const Out e = lower(nullptr, g, S, &op, nullptr);
    CHECK(e.rc == TO_OK && e.run.nz == 0 && e.plants == nullptr && e.run.own_plants.empty() && e.run.pa.mp[0] == 99.0, "own plants, explicit plant: nz %d", e.run.nz);
    // ... unless the handle has per-trajectory time steps: the explicit plant for every sample
    g.dtb = true;
    const Out d = lower(nullptr, g, S, &op, nullptr);
    CHECK(d.rc == TO_OK && d.run.nz == 4 && d.plants == d.run.own_plants.data() && d.run.own_plants.size() == (size_t)16 * S * B && d.run.pa.mp[0] == 99.0, "dtb, explicit plant: nz %d", d.run.nz);
    for (int c = 0; c < S * B && d.run.own_plants.size() == (size_t)16 * S * B; ++c) CHECK(std::memcmp(&d.run.own_plants[(size_t)16 * c], other.data(), sizeof(double) * 16) == 0, "dtb, explicit plant: sample %d", c);
    // per-sample plants of the caller override both
    to_policy_noise z = noise_of(nullptr, nullptr, per_sample.data());
    const Out p = lower(nullptr, g, S, nullptr, &z);
    CHECK(p.rc == TO_OK && p.run.nz == 4 && p.plants == per_sample.data() && p.run.own_plants.empty(), "dtb, per-sample plants");
  }
  { PolicyFacts g = f; g.dtb = true; const Out o = lower(nullptr, g, S, nullptr, nullptr); CHECK(o.rc == TO_OK && o.run.nz == 0 && o.run.own_plants.empty() && o.plants == nullptr, "pm unset: nz %d", o.run.nz); }
  // the clamp
  const double lo[4] = {-1.0, -2.0, -3.0, -4.0}, hi[4] = {1.0, 2.0, 3.0, 4.0};
  {
    to_policy_opts o = kDefault; o.refresh_gains = 0; o.alpha = 0.75; o.u_min = lo;
    const Out r = lower(nullptr, f, 2, &o, nullptr);
    CHECK(r.rc == TO_OK && r.run.pa.clamp == 1 && r.run.pa.alpha == 0.75 && !r.run.refresh_gains, "u_min only");
    for (int j = 0; j < TO_MAX_M; ++j) CHECK(r.run.pa.u_min[j] == (j < 4 ? lo[j] : -HUGE_VAL) && r.run.pa.u_max[j] == HUGE_VAL, "u_min only: [%d]", j);
    o.u_min = nullptr; o.u_max = hi;
    const Out s = lower(nullptr, f, 2, &o, nullptr);
    for (int j = 0; j < TO_MAX_M; ++j) CHECK(s.rc == TO_OK && s.run.pa.clamp == 1 && s.run.pa.u_min[j] == -HUGE_VAL && s.run.pa.u_max[j] == (j < 4 ? hi[j] : HUGE_VAL), "u_max only: [%d]", j);
    o.u_min = hi; o.u_max = hi;  // equal bounds pass
    CHECK(lower(nullptr, f, 2, &o, nullptr).rc == TO_OK, "u_min == u_max");
  }
  // the lane map: TRAJOPT_POLICY_MAP as given, except under force_packed
  {
    PolicyFacts g = f; g.map_env = "uniform"; g.chunk_env = "2";
    const Out u = lower(nullptr, g, 2, nullptr, nullptr), p = lower(nullptr, g, 2, nullptr, nullptr, true);
    CHECK(u.rc == TO_OK && !u.run.packed && u.run.pa.TPW == 0 && u.run.waves == B && u.run.plan.chunk == 2, "uniform by the environment");
    CHECK(p.rc == TO_OK && p.run.packed && p.run.pa.TPW == 32 && p.run.waves == 1 && p.run.plan.chunk == 1, "force_packed ignores the map");
    g.gains_pieces = 5;
    CHECK(lower(nullptr, g, 2, nullptr, nullptr, true).run.plan.lds_bytes == policy_lds_bytes(5, 32), "LDS bytes from the gains pieces");
  }
}

static void mpc_cases() {
  const MpcFacts f{4, "NamedModel", 11, 4};
  const double fill[4] = {0.5, -0.25, 2.0, 1e300};
  auto run = [&](const char* name, const MpcFacts& facts, const to_mpc_opts* o, double* u) {
    double sentinel[TO_MAX_M];
    for (double& v : sentinel) v = kSentinel;
    g_err.clear();
    const int rc = lower_mpc_opts(facts, o, sentinel);
    if (rc != TO_OK) for (double v : sentinel) CHECK(v == kSentinel, "%s: u_fill was touched by a refused call", name);
    if (u) std::memcpy(u, sentinel, sizeof(sentinel));
    printf("case %s code %d msg %s\n", name, rc, rc == TO_OK ? "" : g_err.c_str());
    return rc;
  };
  const to_mpc_opts good = {1, TO_MPC_GUESS_CLOSED_LOOP, TO_MPC_TAIL_FILL, 0, fill};
  run("mpc_null", f, nullptr, nullptr);
  for (int key : {7, 8, 11}) { MpcFacts g = f; g.model_key = key; run(key == 7 ? "mpc_model_7" : key == 8 ? "mpc_model_8" : "mpc_model_11", g, &good, nullptr); }
  { to_mpc_opts o = good; o.shift = 0; run("mpc_shift_low", f, &o, nullptr); }
  { to_mpc_opts o = good; o.shift = 10; run("mpc_shift_high", f, &o, nullptr); }
  { to_mpc_opts o = good; o.guess = 2; run("mpc_guess", f, &o, nullptr); }
  { to_mpc_opts o = good; o.tail = -1; run("mpc_tail", f, &o, nullptr); }
  { to_mpc_opts o = good; o.reserved = 1; run("mpc_reserved", f, &o, nullptr); }
  { to_mpc_opts o = good; o.u_fill = nullptr; run("mpc_fill_null", f, &o, nullptr); }
  { const double bad[4] = {0.0, 0.0, 0.0, Inf}; to_mpc_opts o = good; o.u_fill = bad; run("mpc_fill_not_finite", f, &o, nullptr); }
  { MpcFacts g = f; g.model_key = 9; to_mpc_opts o = good; o.shift = 0; run("order_model_before_shift", g, &o, nullptr); }
  { to_mpc_opts o = good; o.shift = 99; o.guess = 7; o.tail = 7; o.reserved = 7; run("order_shift_before_guess", f, &o, nullptr); }
  { to_mpc_opts o = good; o.reserved = 1; o.u_fill = nullptr; run("order_reserved_before_fill", f, &o, nullptr); }
  double u[TO_MAX_M];
  { to_mpc_opts o = good; o.shift = 9; o.guess = TO_MPC_GUESS_NOMINAL; CHECK(run("mpc_fill", f, &o, u) == TO_OK, "fill"); }
  for (int j = 0; j < TO_MAX_M; ++j) CHECK(u[j] == (j < 4 ? fill[j] : 0.0), "u_fill[%d] = %g", j, u[j]);
  { const double nan_behind_m[4] = {1.0, 2.0, NaN, NaN}; MpcFacts g = f; g.m = 2; to_mpc_opts o = good; o.u_fill = nan_behind_m; CHECK(run("mpc_fill_reads_m_entries", g, &o, u) == TO_OK, "m = 2"); }
  for (int j = 0; j < TO_MAX_M; ++j) CHECK(u[j] == (j == 0 ? 1.0 : j == 1 ? 2.0 : 0.0), "m = 2: u_fill[%d] = %g", j, u[j]);
  { to_mpc_opts o = good; o.tail = TO_MPC_TAIL_HOLD; o.u_fill = nullptr; CHECK(run("mpc_hold", f, &o, u) == TO_OK, "hold"); }
  for (int j = 0; j < TO_MAX_M; ++j) CHECK(u[j] == 0.0, "hold: u_fill[%d] = %g", j, u[j]);
}

int main() {
  policy_refusals();
  policy_outputs();
  mpc_cases();
  printf("fails %d\n", fails);
  return fails ? 1 : 0;
}
