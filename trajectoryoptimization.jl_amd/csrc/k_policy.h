// k_policy.h — closed-loop policy rollouts (to_policy_rollout): S perturbed samples per solved trajectory under the time-varying
// feedback law of the last backward pass,  u = ū_k + α d_k + K_k (x ⊖ x̄_k),  optionally saturated and on a plant whose parameters
// differ from the planning model's.  The operator extends rollout! (src/problem.jl:330-340) / Altro's rollout!(solver, α), which
// apply the same law from the problem's own x0 only.
//
// Lanes are SAMPLES.  Two lane maps share one body (PolicyArgs, common.h):
//   uniform (S > 32)  a wave = 64 samples of ONE trajectory b = wave / WPT.  b comes from blockIdx, so x̄_k, ū_k and the gains row
//                     Kt + (b (N-1) + k) RSK have wave-uniform addresses: they are read once per wave, a knot ahead, through the
//                     constant address space (scalar loads, like the descriptor tables of problem_dev.h) — rows of more than 12
//                     doubles with one vector load per wave (every lane asks for the same address), the Quadrotor's 52-double
//                     row by the forward pass's LDS DMA (stage_gains with one row per wave).
//   packed  (S <= 32) a wave = TPW = 64 / S trajectories x S samples, hardware lane s * TPW + t (the forward pass's map, k_forward.h:
//                     lane t < TPW holds trajectory t, which is what stage_gains expects); per-lane pointers into the tiled nominal.
// Lanes without a sample (tail of the last wave of a trajectory, tail of a packed wave) roll out a copy of a live one and store
// nothing but their own column of the wave's staging block; a sample beyond max_state_value / max_control_value keeps stepping.
// The loop has no lane-divergent region.
//
// NZ (to_policy_rollout_mc; NZ = 0 is to_policy_rollout's kernel, text and code unchanged): bit 0 process noise  x_{k+1} = state_add(f(x_k,
// u_k), w_k), bit 1 measurement noise (the law sees dx_k + v_k; dx_max, J, c_max stay those of the true state and the applied control),
// bit 2 one plant per sample (mp[] loaded per lane from PolicyArgs::plants instead of broadcast from PolicyArgs::mp).  The normals come
// from noise.h, counted by (global trajectory, global sample, k, kind, pair): every lane, dead ones included, draws its own, pair by
// pair as they are consumed — no array of normals is live across the RK step — and the sigmas are wave-uniform kernel arguments.
#pragma once
#include "common.h"
#include "k_forward.h"
#include "noise.h"

// TO_POLICY_HOST (tests/host_shim/policy_harness.cpp compiles this file for the host and runs the kernel thread by thread): the wave's LDS is
// a heap block of exactly the launch's dynamic-LDS bytes (TO_POLICY_HOST_LDS), the DMA of stage_gains a copy that has landed when it returns
// (k_forward.h) and plant parameters stay where they are.  Without the macro nothing below differs from the device text.
#ifdef TO_POLICY_HOST
#define TO_POLICY_LDS(name) double* const name = TO_POLICY_HOST_LDS
#define TO_POLICY_GAINS_LANDED() ((void)0)
#define TO_POLICY_IN_VGPR(x) (x)
#else
#define TO_POLICY_LDS(name) extern __shared__ double name[]
#define TO_POLICY_GAINS_LANDED() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define TO_POLICY_IN_VGPR(x) in_vgpr(x)
#endif

namespace to {

template <bool SC>
__device__ __forceinline__ double policy_ld(const double* p) {
  if constexpr (SC) return *(DoubleC*)p;  // wave-uniform address of data no kernel in flight writes: scalar load
  else return *p;
}

// nominal state / control of one knot and, for the models that do not stage gains through LDS, its gains row
template <class M, bool XSC, bool KSC, bool WITHK>
struct PolicyKnot {
  static constexpr int n = M::n, m = M::m, RSK = Gains<M>::RSK;
  double x[n], u[m], kd[WITHK ? RSK : 1];
  __device__ __forceinline__ void load_x(const double* pXk) {
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = policy_ld<XSC>(&EL(pXk, i));
  }
  __device__ __forceinline__ void load_uk(const double* pUk, const double* pKk) {
#pragma unroll
    for (int j = 0; j < m; ++j) u[j] = policy_ld<XSC>(&EL(pUk, j));
    if constexpr (WITHK) {
#pragma unroll
      for (int i = 0; i < RSK; ++i) kd[i] = policy_ld<KSC>(pKk + i);
    }
  }
};

// objective value of one stage knot; DT (a handle with per-trajectory time steps, DevProblem::dtb): scaled by the trajectory's own step
// GW (a handle with per-trajectory cost weights, DevProblem::gw): the weights of sample c's trajectory b; gw0 = its pointer to entry 0
template <class M, bool DT, bool GW = false>
__device__ __forceinline__ double policy_knot_cost(const DevProblem& P, int k, const double* x, const double* u, const double* gl0, const double* cp0,
                                                   [[maybe_unused]] const double* dt0, [[maybe_unused]] CostLane gw0 = CostLane{nullptr, nullptr}) {
  if constexpr (GW) {
    if constexpr (DT) return knot_cost<M, true>(P, k, x, u, nullptr, nullptr, false, gl0, cp0, nullptr, dt0, gw0);
    else return knot_cost<M, true>(P, k, x, u, nullptr, nullptr, false, gl0, cp0, nullptr, nullptr, gw0);
  } else
  if constexpr (DT) return knot_cost<M, true>(P, k, x, u, nullptr, nullptr, false, gl0, cp0, nullptr, dt0);
  else return knot_cost<M, true>(P, k, x, u, nullptr, nullptr, false, gl0, cp0);
}

// DT: sample c steps by the time steps of ITS trajectory b (DevProblem::dtb).  A handle with per-trajectory steps always runs a one-plant-per-
// sample instance (NZ bit 2), and its launcher picks DT = true (ops.h; problem_dev.h step_dt_of)
template <class M, bool UNIFORM, int FI, int NZ = 0, bool DT = false, bool GW = false>
__global__ void __launch_bounds__(64) k_policy_rollout(KArgs a, PolicyArgs pa) {
  constexpr bool NOISE_W = (NZ & 1) != 0, NOISE_V = (NZ & 2) != 0, LANE_PLANT = (NZ & 4) != 0;
  constexpr int n = M::n, m = M::m, ne = M::ne, RSK = Gains<M>::RSK;
  constexpr bool KLDS = M::lds_gains;
  constexpr bool KSC = UNIFORM && !KLDS && RSK <= 12;
  TO_POLICY_LDS(kbuf);
  const DevProblem& P = a.P;
  const int N = P.N, S = pa.S, hw = threadIdx.x;
  const int g = pa.g0 + blockIdx.x;
  int b, s, t = 0;
  if constexpr (UNIFORM) { b = g / pa.WPT; s = (g - b * pa.WPT) * 64 + hw; }
  else { s = hw / pa.TPW; t = hw - s * pa.TPW; b = g * pa.TPW + t; }
  const bool live = s < S && b < P.B;
  s = s < S ? s : S - 1;
  b = b < P.B ? b : P.B - 1;
  const size_t c = (size_t)b * S + s;  // sample index: sample fastest, then trajectory
  const int tile = b >> 6, lane = b & 63;
  const int TW = UNIFORM ? 1 : pa.TPW;
  const int kbuf_len = KLDS ? gains_lds_doubles<M>(TW) : 0, krow = t * RSK;
  const double* Xc = TILE_PTR(a.Xs, N * n);  // the nominal
  const double* Uc = TILE_PTR(a.Us, (N - 1) * m);
  const double* pK = a.Kt + ((size_t)b * (N - 1)) * RSK;
  // closed-loop states / controls: block [wave of this launch][element][64], every lane its own column (whole 512-byte rows)
  double* pXo = pa.Xw + ((size_t)blockIdx.x * (size_t)(N * n)) * 64 + hw;
  double* pUo = pa.Uw + ((size_t)blockIdx.x * (size_t)((N - 1) * m)) * 64 + hw;
  const double* gl0 = TILE_PTR(P.gl, P.n_costs * (n + m));
  const double* cp0 = TILE_PTR(P.cp, P.n_cp);
  const double* cl0 = TILE_PTR(P.cl, P.n_cl);
  const double* dt0 = dt_lane_of<DT>(P, b);
  [[maybe_unused]] const CostLane gw0 = GW ? cost_lane<n + m>(P, tile, lane) : CostLane{nullptr, nullptr};  // (by the trajectory b, like gl0; weights and attitude references)
  double mp[16];  // the PLANT's parameters; the law's x̄, ū, K, d are the planning model's
  if constexpr (LANE_PLANT) {
    const double* pp = pa.plants + c * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) mp[i] = pp[i];
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) mp[i] = TO_POLICY_IN_VGPR(pa.mp[i]);
  }
  // counter of this lane's draws (noise.h): the GLOBAL trajectory and sample, so that neither the lane map nor a split of the batch
  // over handles or of the samples over calls changes a draw
  [[maybe_unused]] const uint32_t ctraj = pa.traj_offset + (uint32_t)b, csample = pa.sample_offset + (uint32_t)s;
  const int integrator = P.integrator;
  const double max_x = P.opts.max_state_value, max_u = P.opts.max_control_value;
  const double alpha = pa.alpha;
  const bool has_cons = P.n_cons > 0, store = pa.store != 0, clamp = pa.clamp != 0;
  double xb[n];
  {
    const double* px0 = pa.x0s + c * n;
#pragma unroll
    for (int i = 0; i < n; ++i) xb[i] = px0[i];
  }
  if constexpr (KLDS) stage_gains<M>(a.Kt, b, TW, 0, N, kbuf, hw);
  PolicyKnot<M, UNIFORM, KSC, !KLDS> nxt;
  nxt.load_x(Xc);
  nxt.load_uk(Uc, pK);
  const double *pXn = Xc + n * 64, *pUn = Uc + m * 64, *pKn = pK + RSK;  // knot k+1 of the nominal
  double J = 0.0, cm = 0.0, dxm = 0.0;
  int lim = 0, klim = 0;
  for (int k = 0; k < N - 1; ++k) {
    if constexpr (KLDS) TO_POLICY_GAINS_LANDED();  // this knot's gains row has landed in LDS
    const PolicyKnot<M, UNIFORM, KSC, !KLDS> cur = nxt;
    const double* kcur = kbuf + (size_t)(k & 1) * kbuf_len + krow;
    // the next knot's nominal and gains are requested first: nothing issued here is needed before the next iteration
    if (k + 1 < N - 1) {
      if constexpr (KLDS) stage_gains<M>(a.Kt, b, TW, k + 1, N, kbuf + (size_t)((k + 1) & 1) * kbuf_len, hw);
      nxt.load_uk(pUn, pKn);
    }
    nxt.load_x(pXn);  // (k + 1 = N - 1: the terminal knot's x̄, for its |dx|)
    pXn += n * 64; pUn += m * 64; pKn += RSK;
    if (store) {
#pragma unroll
      for (int i = 0; i < n; ++i) EL(pXo, i) = xb[i];
      pXo += n * 64;
    }
    double dx[ne], ub[m], xn[n];
    state_diff<M>(xb, cur.x, dx);
#pragma unroll
    for (int i = 0; i < ne; ++i) { const double v = fabs(dx[i]); if (!(v <= dxm)) dxm = v; }
    if constexpr (NOISE_V) {  // what the law sees: dx_k + v_k (dxm above is the true one)
#pragma unroll
      for (int j = 0; j < (ne + 1) / 2; ++j) {
        double z0, z1;
        normal_pair(pa.seed, ctraj, csample, (uint32_t)k, 1u, (uint32_t)j, &z0, &z1);
        dx[2 * j] += pa.sigma_v[2 * j] * z0;
        if (2 * j + 1 < ne) dx[2 * j + 1] += pa.sigma_v[2 * j + 1] * z1;
      }
    }
#pragma unroll
    for (int j = 0; j < m; ++j) {
      double kr[ne + 1];
#pragma unroll
      for (int i = 0; i <= ne; ++i) kr[i] = KLDS ? kcur[j * (ne + 1) + i] : cur.kd[KLDS ? 0 : j * (ne + 1) + i];
      if constexpr (KLDS) __builtin_amdgcn_sched_barrier(0);
      double du = kr[ne] * alpha;
#pragma unroll
      for (int i = 0; i < ne; ++i) du += kr[i] * dx[i];
      double uj = cur.u[j] + du;
      if (clamp) uj = fmin(fmax(uj, pa.u_min[j]), pa.u_max[j]);  // (wave-uniform branch)
      ub[j] = uj;
      if (store) EL(pUo, j) = uj;
    }
    pUo += m * 64;
    J += policy_knot_cost<M, DT, GW>(P, k, xb, ub, gl0, cp0, dt0, gw0);
    if (has_cons) { const double v = knot_violation<M>(P, k, xb, ub, cp0, cl0); if (!(v <= cm)) cm = v; }
    model_step<M, double, FI>(mp, integrator, k, xb, ub, step_dt_of<DT>(P, k, dt0), xn);
    if constexpr (NOISE_W) {  // x_{k+1} = state_add(f(x_k, u_k), w_k): no dt scaling; the limit test below sees the noisy state
      double w[ne], xf[n];
#pragma unroll
      for (int j = 0; j < (ne + 1) / 2; ++j) {
        double z0, z1;
        normal_pair(pa.seed, ctraj, csample, (uint32_t)k, 0u, (uint32_t)j, &z0, &z1);
        w[2 * j] = pa.sigma_w[2 * j] * z0;
        if (2 * j + 1 < ne) w[2 * j + 1] = pa.sigma_w[2 * j + 1] * z1;
      }
#pragma unroll
      for (int i = 0; i < n; ++i) xf[i] = xn[i];
      state_add<M>(xf, w, xn);
    }
    double mx = 0.0, mu = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) { xb[i] = xn[i]; const double v = fabs(xn[i]); mx = !(v <= mx) ? v : mx; }
#pragma unroll
    for (int j = 0; j < m; ++j) { const double v = fabs(ub[j]); mu = !(v <= mu) ? v : mu; }
    // k_rollout's test: the state the step arrives at first, then the control; the lane keeps stepping (its values are never used)
    const int ev = !(mx <= max_x) ? TO_STATE_LIMIT : !(mu <= max_u) ? TO_CONTROL_LIMIT : 0;
    klim = (lim == 0 && ev != 0) ? k + 1 : klim;
    lim = lim == 0 ? ev : lim;
  }
  {  // terminal knot: nxt.x holds x̄_N
    if (store) {
#pragma unroll
      for (int i = 0; i < n; ++i) EL(pXo, i) = xb[i];
    }
    double dx[ne], u0[m];
    state_diff<M>(xb, nxt.x, dx);
#pragma unroll
    for (int i = 0; i < ne; ++i) { const double v = fabs(dx[i]); if (!(v <= dxm)) dxm = v; }
#pragma unroll
    for (int j = 0; j < m; ++j) u0[j] = 0.0;
    if constexpr (GW) J += knot_cost<M, true>(P, N - 1, xb, u0, nullptr, nullptr, false, gl0, cp0, nullptr, nullptr, gw0);
    else
    J += knot_cost<M, true>(P, N - 1, xb, u0, nullptr, nullptr, false, gl0, cp0);
    if (has_cons) { const double v = knot_violation<M>(P, N - 1, xb, u0, cp0, cl0); if (!(v <= cm)) cm = v; }
  }
  if constexpr (KLDS) TO_POLICY_GAINS_LANDED();
  if (live) {
    const double inf = __builtin_inf();
    pa.J[c] = lim ? inf : J;
    pa.cmax[c] = lim ? inf : cm;
    pa.dxmax[c] = lim ? inf : dxm;
    pa.status[c] = lim;
    pa.klim[c] = klim;
  }
}

}  // namespace to
