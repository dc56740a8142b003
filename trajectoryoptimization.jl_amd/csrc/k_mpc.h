// k_mpc.h — the receding-horizon step on the device (to_mpc_advance): after a closed-loop policy rollout of ONE sample per trajectory
// (k_policy.h at S = 1) the realised state becomes the handle's x0 and the plan moves `s` knots forward, without the closed-loop
// trajectory leaving the device.
//
// Lane map: always the packed map at S = 1 — TPW = 64, wave g = tile g, hardware lane = b & 63.  In that map the staging blocks of
// k_policy_rollout,  Xw[wave - g0][e][64]  and  Uw[wave - g0][e][64],  have the row layout of the tiled nominal arrays,
// base[((b/64) L + e) 64 + b%64]  (common.h): row e of block (g - g0) is row e of tile g.  Every access below is therefore one whole
// 512-byte row of 64 lanes, and nothing is transposed on the way from the rollout to the nominal.
//
// The kernels are copies: no arithmetic touches a value, so what lands in x0 / U is bit for bit what k_policy_rollout stored (or what
// the nominal held).  Plain C++, one wave per workgroup, no LDS.  Non-template: included from trajopt_hip.hip only (and, through the
// host shim, from tests/host_shim/mpc_shift_harness.cpp, which runs the same text under AddressSanitizer).
#pragma once
#include <hip/hip_runtime.h>

namespace to {

constexpr int MPC_MAX_M = 8;  // = TO_MAX_M (include/trajopt_hip.h; static_assert where both are visible)

struct MpcArgs {
  int n, m, N, B;
  int s;       // knots the plan moves forward, 1 <= s <= N - 2
  int guess;   // 0: the applied controls of the rollout become the next guess (written here); 1: the nominal shifted (k_mpc_shift_nominal)
  int tail;    // 0: the s new knots repeat the last control of the chosen sequence; 1: they take u_fill
  int g0;      // first tile of this launch (= PolicyArgs::g0 of the chunk)
  double u_fill[MPC_MAX_M];
  const double* Xw;    // staging of the chunk, [tile - g0][N n][64]
  const double* Uw;    //                       [tile - g0][(N-1) m][64]
  const int* status;   // [B] rollout status of trajectory b (pol_status at S = 1): nonzero -> x0 and U stay as they are
  double* x0;          // tiled, L = n
  double* Us;          // tiled, L = (N-1) m
  // host-layout gather (any may be null): what the entry point downloads
  double* x_next;      // [n, B]
  double* X_applied;   // [n, s+1, B]
  double* U_applied;   // [m, s, B]
};

// x_meas == NULL: the tiled x0 -> the sample-major start states of the policy kernel, pol_x0s[c n + i] with c = b at S = 1.  grid (tiles).
__global__ void __launch_bounds__(64) k_mpc_x0_in(const double* __restrict__ x0, double* __restrict__ x0s, int n, int B) {
  const int tile = blockIdx.x, lane = threadIdx.x, b = tile * 64 + lane;
  if (b >= B) return;
  const double* p = x0 + ((size_t)tile * (size_t)n) * 64 + lane;
  for (int i = 0; i < n; ++i) x0s[(size_t)b * n + i] = p[(size_t)i * 64];
}

// grid (tiles of the chunk, row groups): workgroup (x, y) takes the rows y, y + gridDim.y, ... of tile g0 + x.  A lane behind the batch stores
// nothing (as in k_to_device); a lane whose rollout left the limits gathers what the rollout reported and leaves x0 / U alone.
__global__ void __launch_bounds__(64) k_mpc_writeback(MpcArgs a) {
  const int lane = threadIdx.x, tile = a.g0 + blockIdx.x, b = tile * 64 + lane;
  if (b >= a.B) return;
  const int n = a.n, m = a.m, s = a.s;
  const int Lx = a.N * n, Lu = (a.N - 1) * m;
  const double* xw = a.Xw + ((size_t)blockIdx.x * (size_t)Lx) * 64 + lane;
  const double* uw = a.Uw + ((size_t)blockIdx.x * (size_t)Lu) * 64 + lane;
  const bool ok = a.status[b] == 0;
  const int y0 = blockIdx.y, dy = gridDim.y;
  // the realised state after s steps of the plant: row s n + i of the block
  for (int i = y0; i < n; i += dy) {
    const double v = xw[(size_t)(s * n + i) * 64];
    if (ok) a.x0[((size_t)tile * (size_t)n + i) * 64 + lane] = v;
    if (a.x_next) a.x_next[(size_t)i + (size_t)n * b] = v;
  }
  // closed-loop guess: U[k] = u_cl[k + s], the tail u_cl[N-2] or u_fill.  Reads Uw, writes Us: rows are independent, any split over workgroups will do
  if (a.guess == 0 && ok) {
    double* us = a.Us + ((size_t)tile * (size_t)Lu) * 64 + lane;
    const int keep = Lu - s * m;  // rows that have a source s knots ahead
    for (int e = y0; e < Lu; e += dy) {
      double v;
      if (e < keep) v = uw[(size_t)(e + s * m) * 64];
      else if (a.tail == 0) v = uw[(size_t)(Lu - m + e % m) * 64];
      else v = a.u_fill[e % m];
      us[(size_t)e * 64] = v;
    }
  }
  if (a.X_applied) {
    const int cnt = (s + 1) * n;
    for (int e = y0; e < cnt; e += dy) a.X_applied[(size_t)e + (size_t)cnt * b] = xw[(size_t)e * 64];
  }
  if (a.U_applied) {
    const int cnt = s * m;
    for (int e = y0; e < cnt; e += dy) a.U_applied[(size_t)e + (size_t)cnt * b] = uw[(size_t)e * 64];
  }
}

// Nominal guess: Us shifted IN PLACE, U[k] = Ū[k + s].  A lane's column is read at e + s m and written at e, so rows cannot be split over
// threads: one thread walks its own column in ascending e (the choice made here; the alternative was a copy through the Uw block) and
// every row is read before the walk reaches it.  The hold tail reads the rows of knot N-2, which the walk rewrites last and with their own
// values.  Launched after the policy kernel of the chunk has read the tile (same stream).  grid (tiles of the chunk).
__global__ void __launch_bounds__(64) k_mpc_shift_nominal(MpcArgs a) {
  const int lane = threadIdx.x, tile = a.g0 + blockIdx.x, b = tile * 64 + lane;
  if (b >= a.B || a.status[b] != 0) return;
  const int m = a.m, Lu = (a.N - 1) * m, keep = Lu - a.s * m;
  double* us = a.Us + ((size_t)tile * (size_t)Lu) * 64 + lane;
  for (int e = 0; e < Lu; ++e) {
    double v;
    if (e < keep) v = us[(size_t)(e + a.s * m) * 64];
    else if (a.tail == 0) v = us[(size_t)(Lu - m + e % m) * 64];
    else v = a.u_fill[e % m];
    us[(size_t)e * 64] = v;
  }
}

// ---- to_mpc_shift_duals: the multipliers follow the plan -------------------------------------------------------------------------------
// The tiled dual array (L = n_duals) holds, for constraint ci on knots k1 .. k2 (nk of them, p rows each), the rows
// dual_off + j p + r of knot j = k - k1.  On a trajectory with action 1 (TO_MPC_DUAL_SHIFT)  lam[j] <- lam[j + s]  for j + s < nk, the other
// knots take lam[nk - 1] (tail 0, TO_MPC_DUAL_TAIL_HOLD) or 0 (tail 1, TO_MPC_DUAL_TAIL_ZERO); s >= nk (a terminal constraint: nk = 1): every
// knot is tail.  Action 2 (TO_MPC_DUAL_RESET): lam <- 0 and the constraint's penalty <- mu_reset.  Action 0 (TO_MPC_DUAL_LEAVE), and a lane behind
// the batch, stores nothing.  Penalties are touched by RESET only.
// In place, by the argument of k_mpc_shift_nominal: a lane walks its own column in ascending e, reads row e + s p (not yet written) or, for the
// hold tail, a row of knot nk - 1, which the walk rewrites last and with its own values (s p >= p, so those rows are never shifted into).
// The action picks the value with selects: every lane of the wave issues the same whole-row load and, unless it leaves, the same whole-row store.
struct MpcDualCon {
  long long dual_off;  // DevCon::dual_off
  int p, nk;           // rows per knot, knots (k2 - k1 + 1)
};
struct MpcDualArgs {
  int B, n_cons;
  int s;       // knots the multipliers move forward, >= 1
  int tail;    // 0 hold, 1 zero
  long long n_duals;
  double mu_reset;         // penalty_initial
  const MpcDualCon* cons;  // [n_cons]
  const int* action;       // [B], or null: shift every trajectory
  double* lam;             // tiled, L = n_duals
  double* mu;              // tiled, L = n_cons
};
// grid (tiles, constraints)
__global__ void __launch_bounds__(64) k_mpc_shift_duals(MpcDualArgs a) {
  const int lane = threadIdx.x, tile = blockIdx.x, ci = blockIdx.y, b = tile * 64 + lane;
  if (b >= a.B) return;
  const int act = a.action ? a.action[b] : 1;
  const bool store = act != 0, shift = act == 1;
  const MpcDualCon c = a.cons[ci];
  const int p = c.p, L = p * c.nk;
  const long long d = (long long)a.s * p;
  const int keep = d < L ? (int)(L - d) : 0;  // rows that have a source s knots ahead
  double* lam = a.lam + ((size_t)tile * (size_t)a.n_duals + (size_t)c.dual_off) * 64 + lane;
  for (int e = 0, r = 0; e < L; ++e, r = (r + 1 == p) ? 0 : r + 1) {  // r = e % p
    const bool has = e < keep;
    const int src = has ? e + (int)d : L - p + r;
    double v = lam[(size_t)src * 64];
    v = (has || a.tail == 0) ? v : 0.0;
    v = shift ? v : 0.0;
    if (store) lam[(size_t)e * 64] = v;
  }
  if (act == 2) a.mu[((size_t)tile * (size_t)a.n_cons + (size_t)ci) * 64 + lane] = a.mu_reset;
}

}  // namespace to
