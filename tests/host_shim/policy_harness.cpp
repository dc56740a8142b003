// Compiles csrc/k_policy.h — the closed-loop policy rollout — and csrc/k_mpc.h for the host and runs their kernels thread by thread, wave by
// wave, in the launch sequences of to_policy_rollout and to_mpc_advance (test infrastructure; tests/test_policy_host.py).  The problem is lowered
// from a to_problem_desc with the library's own routines (csrc/desc_lower.h), the lane map, chunk and EVERY buffer length come from the
// library's plan_policy / plan_mpc (csrc/path_plan.h), and every array is allocated with exactly that length: a length that is wrong in the
// library is a heap overflow here.  The kernel has no barrier and no lane-divergent region, so the 64 lanes of a wave run one after another;
// the one thing lanes share, the gains rows in LDS, is copied for the whole wave by stage_gains' host form (k_forward.h, TO_POLICY_HOST).
// Two builds:
//   * a shared object without sanitizers (policy_host_rollout, policy_host_plan, policy_host_solve_path) for the numeric comparison with the
//     restated operator and for the plan queries;
//   * with -DPOLICY_HARNESS_MAIN a stand-alone program, built with -fsanitize=address,undefined, that walks the cases listed at main() on the
//     Quadrotor with the C5 constraint set and a constrained Cartpole, with finite random values (addresses do not depend on values), and
//     prints "checks <count> fails <count>".
// k_policy_to_host (k_generic.h) is restated in to_host() below: k_generic.h holds the multi-wave compaction kernels and is not compiled here.
#define TO_POLICY_HOST 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

struct dim3 { unsigned x = 1, y = 1, z = 1; };
static dim3 blockIdx, threadIdx, gridDim;
#define __launch_bounds__(...)
#define __shared__
// k_policy.h includes k_forward.h for stage_gains: the forward-pass kernels next to it are parsed, never instantiated.  What their text names
// without a template argument needs a declaration to parse; none of these is ever called.
struct double2 { double x, y; };
inline double2 make_double2(double x, double y) { return double2{x, y}; }
void __builtin_amdgcn_fence(int, const char*);
void __builtin_amdgcn_wave_barrier();
void __builtin_amdgcn_s_setprio(int);
void __builtin_amdgcn_s_sleep(int);
void __builtin_amdgcn_s_barrier();
void __syncthreads();
void __threadfence();
void __threadfence_block();
unsigned long long __ballot(int);
int __ffsll(long long);
int atomicAdd(int*, int);
int atomicMax(int*, int);
int atomicOr(int*, int);
int __shfl_xor(int, int);
double __shfl_xor(double, int);
double __shfl(double, int);
int __builtin_amdgcn_readfirstlane(int);
// host forms of what only the device has
static double* g_lds = nullptr;  // the wave's dynamic LDS: a heap block of exactly PolicyPlan::lds_bytes
static int g_wave_b[64];         // the (clamped) trajectory every lane of the running wave holds, from the lane map
#define TO_POLICY_HOST_LDS g_lds
#define TO_POLICY_HOST_LANE_B(t) g_wave_b[t]
inline void __builtin_amdgcn_sched_barrier(int) {}
inline int __shfl(int, int t) { return g_wave_b[t]; }
inline void __builtin_amdgcn_global_load_lds(const void*, void*, int, int, int) {}  // (stage_gains' device branch is compiled out)

#include "k_policy.h"
#include "k_mpc.h"
#include "desc_lower.h"
#include "path_plan.h"

namespace to {
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
}  // namespace to
using namespace to;

// ---- the problem, lowered as to_create lowers it (the tables the policy kernel reads) -----------------------------------------------------
struct Lowered {
  DevProblem P;
  int key = -1;
  std::vector<double> dt;
  std::vector<int> cost_index;
  std::vector<to_cost_desc> costs;
  std::vector<DevCon> cons;
};
static int lower(const to_problem_desc* desc, const to_solver_opts* opts, Lowered* L) {
  int n, m, ne, key;
  if (model_dims(desc->model, desc->model_params, &n, &m, &ne, &key)) return fail(TO_ERR_UNSUPPORTED, "unknown model");
  const int N = desc->N, B = desc->B, Bp = (B + 63) / 64 * 64;
  DevProblem& P = L->P;
  std::memset(&P, 0, sizeof(P));
  L->key = key;
  P.n = n; P.m = m; P.ne = ne; P.N = N; P.B = B; P.Bp = Bp; P.integrator = desc->integrator;
  std::memcpy(P.mp, desc->model_params, sizeof(P.mp));
  if (opts) { int r = validate_opts(*opts); if (r) return r; P.opts = *opts; } else default_opts(&P.opts);
  L->dt.resize(N - 1);
  for (int k = 0; k < N - 1; ++k) L->dt[k] = desc->dt ? desc->dt[k] : (desc->tf - desc->t0) / (N - 1);
  L->cost_index.resize(N);
  for (int k = 0; k < N; ++k) L->cost_index[k] = desc->cost_index ? desc->cost_index[k] : (k == N - 1 ? 1 : 0);
  L->costs.assign(desc->costs, desc->costs + desc->n_costs);
  L->cons.resize(desc->n_constraints);
  long long duals = 0;
  for (int i = 0; i < desc->n_constraints; ++i) {
    int r = validate_constraint(n, m, N, desc->constraints[i], &L->cons[i]);
    if (r) return r;
    L->cons[i].dual_off = duals;
    duals += (long long)L->cons[i].p * (L->cons[i].k2 - L->cons[i].k1 + 1);
  }
  P.n_costs = desc->n_costs; P.n_cons = desc->n_constraints; P.n_duals = duals;
  P.dt = L->dt.data(); P.cost_index = L->cost_index.data(); P.costs = L->costs.data(); P.cons = L->cons.data();
  return TO_OK;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------------
// the run loop of mpc_shift_harness.cpp
template <class K, class... A>
static void run(K kernel, unsigned gx, unsigned gy, const A&... args) {
  gridDim.x = gx; gridDim.y = gy;
  for (blockIdx.y = 0; blockIdx.y < gy; ++blockIdx.y)
    for (blockIdx.x = 0; blockIdx.x < gx; ++blockIdx.x)
      for (threadIdx.x = 0; threadIdx.x < 64; ++threadIdx.x) kernel(args...);
}
// ... and for the policy kernel: before a wave runs, the trajectory of each of its lanes as the kernel's lane map gives it, and its LDS
template <class K>
static void run_policy(K kernel, unsigned waves, const KArgs& a, const PolicyArgs& pa, size_t lds_bytes) {
  gridDim.x = waves; gridDim.y = 1; blockIdx.y = 0;
  std::unique_ptr<double[]> lds(lds_bytes ? new double[lds_bytes / sizeof(double)] : nullptr);
  g_lds = lds.get();
  for (blockIdx.x = 0; blockIdx.x < waves; ++blockIdx.x) {
    const int g = pa.g0 + (int)blockIdx.x;
    for (int hw = 0; hw < 64; ++hw) {
      int b;
      if (pa.TPW == 0) b = g / pa.WPT;
      else { const int s = hw / pa.TPW; b = g * pa.TPW + (hw - s * pa.TPW); }
      g_wave_b[hw] = b < a.P.B ? b : a.P.B - 1;
    }
    for (size_t i = 0; i < lds_bytes / sizeof(double); ++i) lds[i] = -7.0;  // (a wave starts on LDS it has not written)
    for (threadIdx.x = 0; threadIdx.x < 64; ++threadIdx.x) kernel(a, pa);
  }
  g_lds = nullptr;
}
// ops.h op_policy_rollout / with_integrator, ops_policy_mc.hip: the instance of this launch
template <class M, int NZ>
static void launch_policy_nz(const KArgs& a, const PolicyArgs& pa, unsigned waves, size_t lds) {
  static_assert(!M::lds_gains || Gains<M>::RSK % 2 == 0, "whole 16-byte pieces");
  const bool uniform = pa.TPW == 0;
  if constexpr (M::pin_rk4) {
    if (a.P.integrator == INTEG_RK4) {
      if (uniform) run_policy(k_policy_rollout<M, true, INTEG_RK4, NZ>, waves, a, pa, lds);
      else run_policy(k_policy_rollout<M, false, INTEG_RK4, NZ>, waves, a, pa, lds);
      return;
    }
  }
  if (uniform) run_policy(k_policy_rollout<M, true, -1, NZ>, waves, a, pa, lds);
  else run_policy(k_policy_rollout<M, false, -1, NZ>, waves, a, pa, lds);
}
template <class M>
static int launch_policy(const KArgs& a, const PolicyArgs& pa, unsigned waves, int nz, size_t lds) {
  switch (nz) {
    case 0: launch_policy_nz<M, 0>(a, pa, waves, lds); return TO_OK;
    case 4: launch_policy_nz<M, 4>(a, pa, waves, lds); return TO_OK;
    case 7: launch_policy_nz<M, 7>(a, pa, waves, lds); return TO_OK;
  }
  return fail(TO_ERR_UNSUPPORTED, "policy harness: NZ must be 0, 4 or 7");
}
template <class M> constexpr int gains_pieces() { return M::lds_gains ? Gains<M>::RSK / 2 : 0; }

// k_policy_to_host (k_generic.h), restated: staging blocks W[wave - g0][L][64] -> out[e + L (c - c0)] for the samples c0 .. c0 + cnt - 1
static void to_host(const double* W, double* out, int L, int S, int TPW, int WPT, int g0, long long c0, long long cnt) {
  for (long long i = 0; i < cnt; ++i) {
    const long long c = c0 + i;
    const int b = (int)(c / S), s = (int)(c - (long long)b * S);
    const int g = TPW ? b / TPW : b * WPT + s / 64;
    const int lane = TPW ? s * TPW + (b - g * TPW) : s % 64;
    const double* w = W + ((size_t)(g - g0) * (size_t)L) * 64 + lane;
    for (int e = 0; e < L; ++e) out[(size_t)e + (size_t)L * i] = w[(size_t)e * 64];
  }
}

// ---- the handle's arrays a rollout touches, with the lengths to_create and the plan give them ----------------------------------------------
struct Arrays {
  int n, m, ne, N, B, Bp, RSK;
  size_t nXs, nUs, nx0, nKt;
  std::unique_ptr<double[]> Xs, Us, x0, Kt;   // to_create: N n (Bp + 64), (N-1) m Bp, n Bp, Bp (N-1) m (ne+1)
  std::unique_ptr<int[]> st;
  // per call (policy_prepare / policy_staging)
  PolicyPlan pl;
  std::unique_ptr<double[]> x0s, J, cmax, dxmax, plants, xw, uw, stage;
  std::unique_ptr<int[]> status, klim;
};
static double* fresh(std::unique_ptr<double[]>& p, size_t count, double fill) {
  p.reset(count ? new double[count] : nullptr);
  for (size_t i = 0; i < count; ++i) p[i] = fill;
  return p.get();
}
static void make_handle_arrays(const DevProblem& P, Arrays* A) {
  A->n = P.n; A->m = P.m; A->ne = P.ne; A->N = P.N; A->B = P.B; A->Bp = P.Bp; A->RSK = P.m * (P.ne + 1);
  A->nXs = (size_t)P.N * P.n * (P.Bp + 64); A->nUs = (size_t)(P.N - 1) * P.m * P.Bp; A->nx0 = (size_t)P.n * P.Bp;
  A->nKt = (size_t)P.Bp * (P.N - 1) * A->RSK;
  fresh(A->Xs, A->nXs, 0.0); fresh(A->Us, A->nUs, 0.0); fresh(A->x0, A->nx0, 0.0); fresh(A->Kt, A->nKt, 0.0);
}
static double& tiled(double* p, size_t L, int b, size_t e) { return p[((size_t)(b >> 6) * L + e) * 64 + (b & 63)]; }
// nominal [B][N][n] / [B][N-1][m] and gains K [B][N-1][m][ne], d [B][N-1][m] in the host layout -> the device layouts (common.h)
static void set_nominal(Arrays* A, const double* X, const double* U, const double* K, const double* d) {
  const size_t Lx = (size_t)A->N * A->n, Lu = (size_t)(A->N - 1) * A->m;
  for (int b = 0; b < A->B; ++b) {
    for (size_t e = 0; e < Lx; ++e) tiled(A->Xs.get(), Lx, b, e) = X[(size_t)b * Lx + e];
    for (size_t e = 0; e < Lu; ++e) tiled(A->Us.get(), Lu, b, e) = U[(size_t)b * Lu + e];
    for (int i = 0; i < A->n; ++i) tiled(A->x0.get(), A->n, b, i) = X[(size_t)b * Lx + i];
    for (int k = 0; k < A->N - 1; ++k)
      for (int r = 0; r < A->m; ++r) {
        double* row = A->Kt.get() + ((size_t)b * (A->N - 1) + k) * A->RSK + (size_t)r * (A->ne + 1);
        for (int i = 0; i < A->ne; ++i) row[i] = K[(((size_t)b * (A->N - 1) + k) * A->m + r) * A->ne + i];
        row[A->ne] = d[((size_t)b * (A->N - 1) + k) * A->m + r];
      }
  }
}
struct CallOpts {
  int S = 1;
  const char* map_env = nullptr;    // TRAJOPT_POLICY_MAP as the environment would have it
  const char* chunk_env = nullptr;  // TRAJOPT_POLICY_CHUNK_WAVES
  bool force_packed = false;        // to_mpc_advance
  int nz = 0;
  double alpha = 0.0;
  const double *u_min = nullptr, *u_max = nullptr, *plant = nullptr, *plants = nullptr, *sigma_w = nullptr, *sigma_v = nullptr;
  uint64_t seed = 0;
};
constexpr double PATTERN = -12345.678;
// policy_prepare: the argument block and the per-sample arrays
template <class M>
static void prepare(const Lowered& L, Arrays* A, const CallOpts& o, KArgs* a, PolicyArgs* pa) {
  const DevProblem& P = L.P;
  A->pl = plan_policy(P.n, P.m, P.N, P.B, o.S, o.force_packed ? nullptr : o.map_env, o.chunk_env, gains_pieces<M>());
  const PolicyPlan& pl = A->pl;
  std::memset(a, 0, sizeof(*a));
  a->P = P; a->Xs = A->Xs.get(); a->Us = A->Us.get(); a->x0 = A->x0.get(); a->Kt = A->Kt.get();
  std::memset(pa, 0, sizeof(*pa));
  pa->S = o.S; pa->TPW = pl.TPW; pa->WPT = pl.WPT;
  pa->alpha = o.alpha; pa->clamp = (o.u_min || o.u_max) ? 1 : 0;
  for (int j = 0; j < TO_MAX_M; ++j) {
    pa->u_min[j] = (o.u_min && j < P.m) ? o.u_min[j] : -HUGE_VAL;
    pa->u_max[j] = (o.u_max && j < P.m) ? o.u_max[j] : HUGE_VAL;
  }
  std::memcpy(pa->mp, o.plant ? o.plant : P.mp, sizeof(pa->mp));
  for (int i = 0; i < P.ne; ++i) { pa->sigma_w[i] = o.sigma_w ? o.sigma_w[i] : 0.0; pa->sigma_v[i] = o.sigma_v ? o.sigma_v[i] : 0.0; }
  pa->seed = o.seed;
  pa->x0s = fresh(A->x0s, pl.x0s_len, PATTERN);
  pa->J = fresh(A->J, pl.sample_len, PATTERN); pa->cmax = fresh(A->cmax, pl.sample_len, PATTERN); pa->dxmax = fresh(A->dxmax, pl.sample_len, PATTERN);
  A->status.reset(new int[pl.sample_len]); A->klim.reset(new int[pl.sample_len]);
  for (size_t i = 0; i < pl.sample_len; ++i) A->status[i] = A->klim[i] = -99;
  pa->status = A->status.get(); pa->klim = A->klim.get();
  if (o.nz & 4) {
    fresh(A->plants, pl.plants_len, 0.0);
    std::memcpy(A->plants.get(), o.plants, pl.plants_len * sizeof(double));
    pa->plants = A->plants.get();
  } else A->plants.reset();
}
// policy_staging
static void staging(Arrays* A, PolicyArgs* pa) {
  pa->store = 1;
  pa->Xw = fresh(A->xw, A->pl.xw_len, PATTERN); pa->Uw = fresh(A->uw, A->pl.uw_len, PATTERN);
}
// policy_rollout_impl: x0s [B][S][n]; X [B][S][N][n] / U [B][S][N-1][m] or null (the summary-only call: one launch, no staging)
template <class M>
static int rollout(const Lowered& L, Arrays* A, const CallOpts& o, const double* x0s, double* X, double* U) {
  KArgs a; PolicyArgs pa;
  prepare<M>(L, A, o, &a, &pa);
  const PolicyPlan& pl = A->pl;
  std::memcpy(A->x0s.get(), x0s, pl.x0s_len * sizeof(double));
  if (!X && !U) return launch_policy<M>(a, pa, (unsigned)pl.waves, o.nz, pl.lds_bytes);
  staging(A, &pa);
  fresh(A->stage, pl.rollout_stage_len, PATTERN);
  for (long long g0 = 0; g0 < pl.waves; g0 += pl.chunk) {
    const int ng = (int)std::min<long long>(pl.chunk, pl.waves - g0);
    pa.g0 = (int)g0;
    int rc = launch_policy<M>(a, pa, (unsigned)ng, o.nz, pl.lds_bytes);
    if (rc) return rc;
    const long long c0 = policy_first_sample(pl, o.S, g0), cnt = policy_first_sample(pl, o.S, g0 + ng) - c0;
    double* hx = A->stage.get();
    double* hu = A->stage.get() + (size_t)cnt * pl.Lx;
    if (X) { to_host(A->xw.get(), hx, (int)pl.Lx, o.S, pa.TPW, pa.WPT, pa.g0, c0, cnt); std::memcpy(X + (size_t)c0 * pl.Lx, hx, (size_t)cnt * pl.Lx * sizeof(double)); }
    if (U) { to_host(A->uw.get(), hu, (int)pl.Lu, o.S, pa.TPW, pa.WPT, pa.g0, c0, cnt); std::memcpy(U + (size_t)c0 * pl.Lu, hu, (size_t)cnt * pl.Lu * sizeof(double)); }
  }
  return TO_OK;
}
// to_mpc_advance up to its closing rollout: x_meas [B][n] or null; out arrays in the C-ABI's layout, any may be null
struct MpcOut { double *x_next = nullptr, *X_applied = nullptr, *U_applied = nullptr; };
template <class M>
static int advance(const Lowered& L, Arrays* A, CallOpts o, const double* x_meas, int s, int guess, int tail, const double* u_fill, const MpcOut& out) {
  const DevProblem& P = L.P;
  o.S = 1; o.force_packed = true;
  MpcArgs ma;
  std::memset(&ma, 0, sizeof(ma));
  if (tail == 1) for (int j = 0; j < P.m; ++j) ma.u_fill[j] = u_fill[j];
  KArgs a; PolicyArgs pa;
  prepare<M>(L, A, o, &a, &pa);
  const PolicyPlan& pl = A->pl;
  staging(A, &pa);
  const MpcPlan mp = plan_mpc(P.n, P.m, P.N, P.B, s);
  fresh(A->stage, mp.stage_len, PATTERN);
  ma.n = P.n; ma.m = P.m; ma.N = P.N; ma.B = P.B; ma.s = s; ma.guess = guess; ma.tail = tail;
  ma.Xw = A->xw.get(); ma.Uw = A->uw.get(); ma.status = A->status.get(); ma.x0 = A->x0.get(); ma.Us = A->Us.get();
  ma.x_next = out.x_next ? A->stage.get() : nullptr;
  ma.X_applied = out.X_applied ? A->stage.get() + mp.cx : nullptr;
  ma.U_applied = out.U_applied ? A->stage.get() + mp.cx + mp.cX : nullptr;
  if (x_meas) std::memcpy(A->x0s.get(), x_meas, mp.cx * sizeof(double));
  else run(k_mpc_x0_in, (unsigned)pl.waves, 1u, (const double*)A->x0.get(), A->x0s.get(), P.n, P.B);
  for (long long g0 = 0; g0 < pl.waves; g0 += pl.chunk) {
    const int ng = (int)std::min<long long>(pl.chunk, pl.waves - g0);
    pa.g0 = ma.g0 = (int)g0;
    int rc = launch_policy<M>(a, pa, (unsigned)ng, o.nz, pl.lds_bytes);
    if (rc) return rc;
    run(k_mpc_writeback, (unsigned)ng, (unsigned)mp.row_groups, ma);
    if (guess == 1) run(k_mpc_shift_nominal, (unsigned)ng, 1u, ma);
  }
  if (ma.x_next) std::memcpy(out.x_next, ma.x_next, mp.cx * sizeof(double));
  if (ma.X_applied) std::memcpy(out.X_applied, ma.X_applied, mp.cX * sizeof(double));
  if (ma.U_applied) std::memcpy(out.U_applied, ma.U_applied, mp.cU * sizeof(double));
  return TO_OK;
}

// ---- the shared object's interface (ctypes) -----------------------------------------------------------------------------------------------
extern "C" const char* policy_host_last_error() { return g_err.c_str(); }

// lane_map: 0 the library's choice, 1 TRAJOPT_POLICY_MAP=packed, 2 =uniform; chunk_waves: 0 the library's, else TRAJOPT_POLICY_CHUNK_WAVES.
// Xbar [B][N][n], Ubar [B][N-1][m], K [B][N-1][m][ne], d [B][N-1][m], x0s [B][S][n]; results sample fastest, then trajectory; X / U may be null.
extern "C" int policy_host_rollout(const to_problem_desc* desc, const to_solver_opts* opts, int S, int lane_map, int chunk_waves, const double* Xbar,
                                   const double* Ubar, const double* K, const double* d, const double* x0s, double alpha, const double* u_min,
                                   const double* u_max, const double* plant, double* X, double* U, double* J, double* cmax, double* dxmax,
                                   int32_t* status, int32_t* klim) {
  Lowered L;
  int rc = lower(desc, opts, &L);
  if (rc) return rc;
  Arrays A;
  make_handle_arrays(L.P, &A);
  set_nominal(&A, Xbar, Ubar, K, d);
  CallOpts o;
  const std::string chunk = std::to_string(chunk_waves);
  o.S = S; o.map_env = lane_map == 1 ? "packed" : lane_map == 2 ? "uniform" : nullptr; o.chunk_env = chunk_waves ? chunk.c_str() : nullptr;
  o.alpha = alpha; o.u_min = u_min; o.u_max = u_max; o.plant = plant;
  switch (L.key) {
    case 1: rc = rollout<DoubleIntegratorModel<2>>(L, &A, o, x0s, X, U); break;
    case 3: rc = rollout<CartpoleModel>(L, &A, o, x0s, X, U); break;
    case 4: rc = rollout<QuadrotorModel>(L, &A, o, x0s, X, U); break;
    default: return fail(TO_ERR_UNSUPPORTED, "policy harness: model not instantiated");
  }
  if (rc) return rc;
  const size_t SB = A.pl.SB;
  std::memcpy(J, A.J.get(), SB * sizeof(double)); std::memcpy(cmax, A.cmax.get(), SB * sizeof(double)); std::memcpy(dxmax, A.dxmax.get(), SB * sizeof(double));
  std::memcpy(status, A.status.get(), SB * sizeof(int32_t)); std::memcpy(klim, A.klim.get(), SB * sizeof(int32_t));
  return TO_OK;
}

// plan_policy / plan_mpc as the entry points call them: out[0..12) = packed, TPW, WPT, waves, SB, x0s_len, sample_len, chunk, xw_len, uw_len,
// rollout_stage_len, lds_bytes; mpc[0..5) = cx, cX, cU, stage_len, row_groups (shift s)
extern "C" void policy_host_plan(int n, int m, int N, int B, int S, int lane_map, int chunk_waves, int gains_pieces_, int s, long long* out, long long* mpc) {
  const std::string chunk = std::to_string(chunk_waves);
  const PolicyPlan p = plan_policy(n, m, N, B, S, lane_map == 1 ? "packed" : lane_map == 2 ? "uniform" : nullptr, chunk_waves ? chunk.c_str() : nullptr, gains_pieces_);
  const long long v[12] = {p.packed, p.TPW, p.WPT, p.waves, (long long)p.SB, (long long)p.x0s_len, (long long)p.sample_len, p.chunk, (long long)p.xw_len,
                           (long long)p.uw_len, (long long)p.rollout_stage_len, (long long)p.lds_bytes};
  std::memcpy(out, v, sizeof(v));
  const MpcPlan q = plan_mpc(n, m, N, B, s);
  const long long w[5] = {(long long)q.cx, (long long)q.cX, (long long)q.cU, (long long)q.stage_len, q.row_groups};
  std::memcpy(mpc, w, sizeof(w));
}

// Which kernels a constrained Quadrotor handle of B trajectories runs on `cus` compute units (path_plan.h plan_paths / plan_step with the Quadrotor's
// launch-table traits, as tests/host_shim/path_plan_harness.cpp has them): info[0..8) = to_solver_path's report; step[0..6) = the first batch step's
// kind, CW, TW, two_wave, store_x, two_launch at last_active = `active`
extern "C" void policy_host_solve_path(int B, int N, int cus, int active, int32_t* info, int32_t* step) {
  PathTraits t;
  t.write_through = false; t.mfma_backward = true; t.coop_backward = false; t.lane_backward = false; t.ls_first_round = 16;
  t.accept_roll = true; t.expand_const = true;
  t.forward = t.forward2 = 0x0F0Fu | (3u << 18) | (3u << 26); t.forward_plants = (1u << 8) | (1u << 10);
  PathShape s;
  s.B = B; s.Bp = (B + 63) / 64 * 64; s.N = N; s.ne = 12; s.m = 4; s.n_cons = 2; s.iterations_linesearch = 20; s.diagonal_cost_blocks = false; s.cus = cus;
  const PathKnobs k = read_path_knobs([](const char*) -> const char* { return nullptr; });
  const PathPlan p = plan_paths(t, s, k);
  path_report(p, t, 0, 2, B, info);
  const StepPlan sp = plan_step(p, t, 0, 2, solve_compact(p), active, B);
  step[0] = sp.kind; step[1] = sp.CW; step[2] = sp.TW; step[3] = sp.two_wave; step[4] = sp.store_x; step[5] = sp.two_launch;
}

#ifdef POLICY_HARNESS_MAIN
// ---- the sanitized program ----------------------------------------------------------------------------------------------------------------
static long long g_checks = 0, g_fails = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double unit() {  // uniform in [-1, 1)
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) * 0x1p-52 - 1.0;
}
static std::string g_case;
static void expect(bool ok, const char* what, long long at = 0) {
  ++g_checks;
  if (ok) return;
  if (++g_fails <= 30) std::printf("FAIL %s at %lld: %s\n", what, at, g_case.c_str());
}
static bool same(const double* a, const double* b, size_t count) { return count == 0 || std::memcmp(a, b, count * sizeof(double)) == 0; }
static bool same(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && same(a.data(), b.data(), a.size()); }

// the two problems, built from the public header's structs
struct Built {
  to_problem_desc desc;
  std::vector<to_cost_desc> costs;
  std::vector<to_constraint_desc> cons;
};
static void quadrotor_c5(int N, int B, Built* b) {
  std::memset(&b->desc, 0, sizeof(b->desc));
  b->costs.assign(2, to_cost_desc{});
  b->cons.assign(2, to_constraint_desc{});
  const double xf[13] = {2.0, 3.0, 1.0, 0.3826834323650898, 0.0, 0.0, 0.9238795325112867, 0, 0, 0, 0, 0, 0};
  const double Qd[13] = {1, 1, 1, 0, 0, 0, 0, .1, .1, .1, .1, .1, .1};
  for (int c = 0; c < 2; ++c) {  // DiagonalQuatCost: 0.5 (x - xf)' Q (x - xf) as Q, q = -Q xf, c; + w min(1 -/+ q_ref' q)
    to_cost_desc& C = b->costs[c];
    C.kind = TO_COST_DIAGONAL_QUAT; C.terminal = c;
    for (int i = 0; i < 13; ++i) { C.Q[i] = (c ? 100.0 : 1.0) * Qd[i]; C.q[i] = -C.Q[i] * xf[i]; }
    for (int j = 0; j < 4; ++j) { C.R[j] = 1e-2; C.r[j] = -1e-2 * 1.22625; }
    C.w = 1.0;
    for (int i = 0; i < 4; ++i) { C.q_ref[i] = xf[3 + i]; C.q_ind[i] = 4 + i; }
  }
  to_constraint_desc& soc = b->cons[0];  // NormConstraint |u| <= 6, second-order cone, knots 1 .. N-1
  soc.kind = TO_CON_NORM; soc.sense = TO_CONE_SECOND_ORDER; soc.k_first = 1; soc.k_last = N - 1; soc.n_inds = 4;
  for (int j = 0; j < 4; ++j) soc.inds[j] = 13 + j + 1;
  soc.n_params = 1; soc.params[0] = 6.0;
  to_constraint_desc& goal = b->cons[1];  // GoalConstraint on C5_GOAL_INDS, knot N
  const int inds[9] = {1, 2, 3, 8, 9, 10, 11, 12, 13};
  goal.kind = TO_CON_GOAL; goal.sense = TO_CONE_ZERO; goal.k_first = goal.k_last = N; goal.n_inds = goal.n_params = 9;
  for (int i = 0; i < 9; ++i) { goal.inds[i] = inds[i]; goal.params[i] = xf[inds[i] - 1]; }
  to_problem_desc& d = b->desc;
  d.abi_version = TO_ABI_VERSION; d.model = TO_MODEL_QUADROTOR; d.integrator = TO_RK4; d.n = 13; d.m = 4; d.N = N; d.B = B;
  const double mp[11] = {0.5, 0.0023, 0.0023, 0.004, 0.0, 0.0, -9.81, 0.1750, 1.0, 0.0245, 0.0};
  std::memcpy(d.model_params, mp, sizeof(mp));
  d.t0 = 0.0; d.tf = 0.05 * (N - 1);
  d.n_costs = 2; d.costs = b->costs.data(); d.n_constraints = 2; d.constraints = b->cons.data();
}
static void cartpole_constrained(int N, int B, Built* b) {
  std::memset(&b->desc, 0, sizeof(b->desc));
  b->costs.assign(2, to_cost_desc{});
  b->cons.assign(2, to_constraint_desc{});
  for (int c = 0; c < 2; ++c) {
    to_cost_desc& C = b->costs[c];
    C.kind = TO_COST_DIAGONAL; C.terminal = c;
    for (int i = 0; i < 4; ++i) { C.Q[i] = c ? 100.0 : 0.01; C.q[i] = i == 1 ? -C.Q[i] * 3.141592653589793 : 0.0; }
    C.R[0] = 0.1;
  }
  to_constraint_desc& bnd = b->cons[0];  // BoundConstraint |u| <= 3 on 1 .. N-1
  bnd.kind = TO_CON_BOUND; bnd.sense = TO_CONE_NEGATIVE_ORTHANT; bnd.k_first = 1; bnd.k_last = N - 1; bnd.n_params = 10;
  for (int i = 0; i < 5; ++i) { bnd.params[i] = i == 4 ? 3.0 : HUGE_VAL; bnd.params[5 + i] = i == 4 ? -3.0 : -HUGE_VAL; }
  to_constraint_desc& goal = b->cons[1];
  goal.kind = TO_CON_GOAL; goal.sense = TO_CONE_ZERO; goal.k_first = goal.k_last = N; goal.n_inds = goal.n_params = 4;
  for (int i = 0; i < 4; ++i) { goal.inds[i] = i + 1; goal.params[i] = i == 1 ? 3.141592653589793 : 0.0; }
  to_problem_desc& d = b->desc;
  d.abi_version = TO_ABI_VERSION; d.model = TO_MODEL_CARTPOLE; d.integrator = TO_RK4; d.n = 4; d.m = 1; d.N = N; d.B = B;
  const double mp[4] = {1.0, 0.2, 0.5, 9.81};
  std::memcpy(d.model_params, mp, sizeof(mp));
  d.t0 = 0.0; d.tf = 0.05 * (N - 1);
  d.n_costs = 2; d.costs = b->costs.data(); d.n_constraints = 2; d.constraints = b->cons.data();
}

// finite random nominal, gains and start states near a plausible operating point (every lane steps through finite numbers; every fifth
// trajectory's samples start beyond max_state_value, so both outcomes of the limit test are there)
struct Inputs { std::vector<double> X, U, K, d, x0s, plants; };
static void random_inputs(const DevProblem& P, int S, Inputs* in) {
  const int n = P.n, m = P.m, ne = P.ne, N = P.N, B = P.B;
  const bool quad = n == 13;
  in->X.resize((size_t)B * N * n); in->U.resize((size_t)B * (N - 1) * m);
  in->K.resize((size_t)B * (N - 1) * m * ne); in->d.resize((size_t)B * (N - 1) * m);
  in->x0s.resize((size_t)B * S * n); in->plants.resize((size_t)B * S * 16);
  auto state = [&](double* x, double spread) {
    for (int i = 0; i < n; ++i) x[i] = spread * unit();
    if (quad) { x[3] = 1.0 + 0.1 * unit(); }
  };
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < N; ++k) state(&in->X[((size_t)b * N + k) * n], 0.5);
    for (size_t i = 0; i < (size_t)(N - 1) * m; ++i) in->U[(size_t)b * (N - 1) * m + i] = (quad ? 1.2 : 0.0) + 0.3 * unit();
    for (int s = 0; s < S; ++s) {
      double* x = &in->x0s[((size_t)b * S + s) * n];
      state(x, 0.5);
      if (b % 5 == 3) x[0] = 1e9;
      double* pp = &in->plants[((size_t)b * S + s) * 16];
      for (int i = 0; i < 16; ++i) pp[i] = P.mp[i] * (i == 0 ? 1.0 + 0.1 * unit() : 1.0);
    }
  }
  for (double& v : in->K) v = 0.05 * unit();
  for (double& v : in->d) v = 0.1 * unit();
}
struct Results {
  std::vector<double> X, U, J, cmax, dxmax;
  std::vector<int> status, klim;
};
static void take_summaries(const Arrays& A, Results* r) {
  const size_t SB = A.pl.SB;
  r->J.assign(A.J.get(), A.J.get() + SB); r->cmax.assign(A.cmax.get(), A.cmax.get() + SB); r->dxmax.assign(A.dxmax.get(), A.dxmax.get() + SB);
  r->status.assign(A.status.get(), A.status.get() + SB); r->klim.assign(A.klim.get(), A.klim.get() + SB);
}
static void check_same_results(const Results& a, const Results& b, bool with_traj, const char* what) {
  expect(same(a.J, b.J) && same(a.cmax, b.cmax) && same(a.dxmax, b.dxmax) && a.status == b.status && a.klim == b.klim, what);
  if (with_traj) expect(same(a.X, b.X) && same(a.U, b.U), what, 1);
}

// to_policy_rollout on one (problem, S, NZ): every lane map that can serve, chunks of one wave and of all waves, with and without the trajectories.
// All of them must give the same bits (the lane map and the chunking change no arithmetic), leave the handle's arrays as they were and write
// every per-sample entry.
template <class M>
static void rollout_cases(const Lowered& L, int S, int nz, bool all_variants) {
  const DevProblem& P = L.P;
  Arrays A;
  make_handle_arrays(P, &A);
  Inputs in;
  random_inputs(P, S, &in);
  set_nominal(&A, in.X.data(), in.U.data(), in.K.data(), in.d.data());
  // lanes behind the batch and the spare tile hold a pattern too: nothing may depend on them, nothing may write them
  const std::vector<double> Xs0(A.Xs.get(), A.Xs.get() + A.nXs), Us0(A.Us.get(), A.Us.get() + A.nUs), x00(A.x0.get(), A.x0.get() + A.nx0),
      Kt0(A.Kt.get(), A.Kt.get() + A.nKt);
  std::vector<double> sw(P.ne, 1e-3), sv(P.ne, 1e-3);
  Results first;
  bool have = false;
  const char* maps[3] = {nullptr, "packed", "uniform"};
  for (int mi = 0; mi < 3; ++mi) {
    if (mi == 1 && (S > 64 || S <= 32)) continue;  // (packed cannot serve / is the default already)
    if (mi == 2 && S > 32) continue;               // (uniform is the default already)
    if (mi && !all_variants) continue;
    if (mi == 2 && (P.B > 65 || (P.B == 65 && P.N > 4))) continue;  // (a forced uniform map spends a whole wave per sample: kept to the small shapes)
    for (int chunk_all = 0; chunk_all < 2; ++chunk_all)
      for (int store = 0; store < 2; ++store) {
        if (!store && chunk_all) continue;  // (the summary-only call has no chunks)
        if (!all_variants && !(store && !chunk_all)) continue;
        CallOpts o;
        o.S = S; o.map_env = maps[mi]; o.chunk_env = chunk_all ? nullptr : "1"; o.nz = nz; o.alpha = 0.5;
        if (nz & 1) o.sigma_w = sw.data();
        if (nz & 2) o.sigma_v = sv.data();
        if (nz & 4) o.plants = in.plants.data();
        o.seed = 0x1234abcdull;
        g_case = "rollout n " + std::to_string(P.n) + " N " + std::to_string(P.N) + " B " + std::to_string(P.B) + " S " + std::to_string(S) + " nz " +
                 std::to_string(nz) + " map " + (maps[mi] ? maps[mi] : "default") + (chunk_all ? " all waves" : " one wave") + (store ? " store" : " summaries");
        Results r;
        const size_t SB = (size_t)S * P.B;
        if (store) { r.X.assign(SB * P.N * P.n, PATTERN); r.U.assign(SB * (P.N - 1) * P.m, PATTERN); }
        const int rc = rollout<M>(L, &A, o, in.x0s.data(), store ? r.X.data() : nullptr, store ? r.U.data() : nullptr);
        expect(rc == TO_OK, "rollout returned an error");
        if (rc) continue;
        take_summaries(A, &r);
        expect(chunk_all || !store || A.pl.chunk == 1, "chunk of one wave");
        expect(same(A.Xs.get(), Xs0.data(), A.nXs) && same(A.Us.get(), Us0.data(), A.nUs) && same(A.x0.get(), x00.data(), A.nx0) &&
                   same(A.Kt.get(), Kt0.data(), A.nKt), "the handle's arrays are read only");
        expect(same(A.x0s.get(), in.x0s.data(), A.pl.x0s_len), "start states are read only");
        bool written = true, limits = true;
        for (size_t c = 0; c < SB; ++c) {
          written = written && r.status[c] != -99 && r.klim[c] != -99 && r.J[c] != PATTERN && r.cmax[c] != PATTERN && r.dxmax[c] != PATTERN;
          const bool far = (c / S) % 5 == 3;  // started beyond max_state_value
          limits = limits && (far ? r.status[c] != 0 : true);
        }
        expect(written, "every sample has its results");
        expect(limits, "samples that start beyond the limit report it");
        if (store) {
          bool all_set = true;
          for (double v : r.X) all_set = all_set && v != PATTERN;
          for (double v : r.U) all_set = all_set && v != PATTERN;
          expect(all_set, "every sample's trajectory is handed over");
          // sample c's first state is its start state
          bool starts = true;
          for (size_t c = 0; c < SB; ++c) starts = starts && same(&r.X[c * P.N * P.n], &in.x0s[c * P.n], P.n);
          expect(starts, "knot 1 of every sample is its start state");
        }
        if (!have && store) { first = r; have = true; }
        else if (have) check_same_results(first, r, store, "lane maps, chunkings and the summary-only call agree bit for bit");
      }
  }
}

// to_mpc_advance on one (problem, s, guess, tail, chunking): the expected values come from the closed-loop trajectories of to_policy_rollout
// at S = 1 on the same handle arrays (whose lane-map independence rollout_cases checks) and the plain loops of mpc_shift_harness.cpp.
template <class M>
static void advance_cases(const Lowered& L, int nz) {
  const DevProblem& P = L.P;
  const int n = P.n, m = P.m, N = P.N, B = P.B;
  const size_t Lx = (size_t)N * n, Lu = (size_t)(N - 1) * m;
  Inputs in;
  random_inputs(P, 1, &in);
  const int shifts[2] = {1, N - 2};
  for (int si = 0; si < 2; ++si)
    for (int guess = 0; guess < 2; ++guess)
      for (int tail = 0; tail < 2; ++tail)
        for (int chunk_all = 0; chunk_all < 2; ++chunk_all)
          for (int meas = 0; meas < 2; ++meas) {
            const int s = shifts[si];
            if (si == 1 && N - 2 == 1) continue;
            // every combination at NZ = 0 up to B = 130; the large batch without x_meas and with the tail that goes with the guess; the stochastic
            // instances (the same addresses but for the plants) on four combinations that still hold every value of every switch
            if (nz == 0 && B > 130 && (meas == 1 || tail != guess)) continue;
            if (nz != 0 && (tail != guess || chunk_all != si || meas != guess)) continue;
            g_case = "advance n " + std::to_string(n) + " N " + std::to_string(N) + " B " + std::to_string(B) + " nz " + std::to_string(nz) + " s " + std::to_string(s) +
                     " guess " + std::to_string(guess) + " tail " + std::to_string(tail) + (chunk_all ? " all waves" : " one wave") + (meas ? " x_meas" : " x0");
            Arrays A;
            make_handle_arrays(P, &A);
            for (size_t i = 0; i < A.nXs; ++i) A.Xs[i] = 0.25 * unit();  // lanes behind the batch hold values of their own
            for (size_t i = 0; i < A.nUs; ++i) A.Us[i] = 0.25 * unit();
            for (size_t i = 0; i < A.nx0; ++i) A.x0[i] = 0.25 * unit();
            for (size_t i = 0; i < A.nKt; ++i) A.Kt[i] = 0.01 * unit();
            set_nominal(&A, in.X.data(), in.U.data(), in.K.data(), in.d.data());
            if (!meas)  // the handle's x0 are the start states (k_mpc_x0_in)
              for (int b = 0; b < B; ++b) for (int i = 0; i < n; ++i) tiled(A.x0.get(), n, b, i) = in.x0s[(size_t)b * n + i];
            const std::vector<double> Xs0(A.Xs.get(), A.Xs.get() + A.nXs), Us0(A.Us.get(), A.Us.get() + A.nUs), x00(A.x0.get(), A.x0.get() + A.nx0),
                Kt0(A.Kt.get(), A.Kt.get() + A.nKt);
            CallOpts o;
            o.nz = nz; o.alpha = 0.5; o.seed = 77; o.chunk_env = chunk_all ? nullptr : "1";
            std::vector<double> sw(P.ne, 1e-3), sv(P.ne, 1e-3);
            if (nz & 1) o.sigma_w = sw.data();
            if (nz & 2) o.sigma_v = sv.data();
            if (nz & 4) o.plants = in.plants.data();
            // reference: the closed loop of every trajectory, through to_policy_rollout's sequence (default map at S = 1: packed)
            Results ref;
            ref.X.assign((size_t)B * Lx, PATTERN); ref.U.assign((size_t)B * Lu, PATTERN);
            CallOpts oref = o;
            oref.S = 1; oref.chunk_env = nullptr;
            expect(rollout<M>(L, &A, oref, in.x0s.data(), ref.X.data(), ref.U.data()) == TO_OK, "reference rollout");
            take_summaries(A, &ref);
            double fill[TO_MAX_M];
            for (int j = 0; j < TO_MAX_M; ++j) fill[j] = unit();
            std::vector<double> x_next((size_t)n * B, PATTERN), Xa((size_t)n * (s + 1) * B, PATTERN), Ua((size_t)m * s * B, PATTERN);
            MpcOut out;
            out.x_next = x_next.data(); out.X_applied = Xa.data(); out.U_applied = Ua.data();
            const int rc = advance<M>(L, &A, o, meas ? in.x0s.data() : nullptr, s, guess, tail, fill, out);
            expect(rc == TO_OK, "advance returned an error");
            if (rc) continue;
            Results got;
            take_summaries(A, &got);
            check_same_results(ref, got, false, "summaries of the advance equal those of the rollout");
            expect(same(A.Xs.get(), Xs0.data(), A.nXs) && same(A.Kt.get(), Kt0.data(), A.nKt), "nominal states and gains are read only");
            bool moved_any = false, kept_any = false;
            for (int b = 0; b < A.Bp; ++b) {
              const bool moved = b < B && ref.status[b] == 0;
              moved_any = moved_any || moved; kept_any = kept_any || (b < B && !moved);
              for (int i = 0; i < n; ++i) {
                const double want = moved ? ref.X[(size_t)b * Lx + (size_t)s * n + i] : tiled(const_cast<double*>(x00.data()), n, b, i);
                expect(same(&tiled(A.x0.get(), n, b, i), &want, 1), moved ? "x0" : "x0 kept", b);
              }
              for (int k = 0; k < N - 1; ++k)
                for (int j = 0; j < m; ++j) {
                  auto V = [&](int kk) { return guess == 0 ? ref.U[(size_t)b * Lu + (size_t)kk * m + j] : tiled(const_cast<double*>(Us0.data()), Lu, b, (size_t)kk * m + j); };
                  double want = tiled(const_cast<double*>(Us0.data()), Lu, b, (size_t)k * m + j);
                  if (moved) want = k + s <= N - 2 ? V(k + s) : tail == 0 ? V(N - 2) : fill[j];
                  expect(same(&tiled(A.Us.get(), Lu, b, (size_t)k * m + j), &want, 1), moved ? "U" : "U kept", b);
                }
              if (b >= B) continue;
              expect(same(&x_next[(size_t)n * b], &ref.X[(size_t)b * Lx + (size_t)s * n], n), "x_next", b);
              expect(same(&Xa[(size_t)n * (s + 1) * b], &ref.X[(size_t)b * Lx], (size_t)n * (s + 1)), "X_applied", b);
              expect(same(&Ua[(size_t)m * s * b], &ref.U[(size_t)b * Lu], (size_t)m * s), "U_applied", b);
            }
            expect(moved_any, "some trajectory completes its rollout");
            expect(kept_any || B < 4, "some trajectory leaves the limits");
          }
}

template <class M>
static void model_cases(void (*build)(int, int, Built*), const int* nzs, int n_nz) {
  const int Ns[2] = {4, 21}, Bs[5] = {1, 64, 65, 130, 1024}, Ss[5] = {1, 3, 33, 64, 70};
  for (int N : Ns)
    for (int B : Bs) {
      Built built;
      build(N, B, &built);
      Lowered L;
      const int rc = lower(&built.desc, nullptr, &L);
      g_case = "lowering";
      expect(rc == TO_OK, g_err.c_str());
      if (rc) continue;
      for (int zi = 0; zi < n_nz; ++zi) {
        // every (S, map, chunking, store) with NZ = 0; the stochastic instances share the addresses of everything but the plants: one variant each.
        // Every S at B = 1 and 65 (one lane, one lane behind a full tile); 1, 3, 70 at 130; the packed sizes at 64; the batch that faulted, 1024, at
        // S = 1, the shape to_mpc_advance runs (16 waves): the work grows with S * B and the addresses repeat from tile to tile.
        for (int S : Ss) {
          const bool run_it = B == 1 || B == 65 || (B == 130 && (S <= 3 || S == 70)) || (B == 64 && S <= 3) || (B == 1024 && S == 1);
          if (run_it) rollout_cases<M>(L, S, nzs[zi], nzs[zi] == 0);
        }
        advance_cases<M>(L, nzs[zi]);
      }
    }
}

int main() {
  const int quad_nz[3] = {0, 4, 7}, cart_nz[1] = {0};
  model_cases<QuadrotorModel>(quadrotor_c5, quad_nz, 3);
  model_cases<CartpoleModel>(cartpole_constrained, cart_nz, 1);
  std::printf("checks %lld fails %lld\n", g_checks, g_fails);
  return g_fails == 0 ? 0 : 1;
}
#endif
