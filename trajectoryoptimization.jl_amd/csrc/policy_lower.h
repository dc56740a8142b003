// policy_lower.h — what to_policy_rollout, to_policy_rollout_mc and to_mpc_advance check and compute on the host before their first device
// call.  Pure host C++ over small Facts structs (no handle), like desc_lower.h; tests/host_shim/policy_lower_harness.cpp runs it on the CPU.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "common.h"  // PolicyArgs
#include "desc_lower.h"
#include "path_plan.h"

namespace to {

// One closed-loop rollout as its three entry points share it: the validated options as the kernel's argument block, the kernel instance, the
// lane map and the plan (lower_policy_opts: the host half; trajopt_hip.hip policy_prepare: the device pointers, policy_staging: the staging pair).
struct PolicyRun {
  PolicyArgs pa;
  int nz = 0;          // the kernel's NZ: bit 0 process noise, bit 1 measurement noise, bit 2 one plant per sample
  bool packed = true;  // lane map
  int waves = 0;
  size_t SB = 0;
  PolicyPlan plan;     // every length below comes from here (path_plan.h plan_policy)
  std::vector<double> own_plants;  // the handle's per-trajectory plants repeated per sample (alive until the entry point returns)
  bool refresh_gains = true;       // to_policy_opts::refresh_gains, validated
};
// What lower_policy_opts reads of a handle (model_key as in TrackFacts).
struct PolicyFacts {
  int model_key; const double* mp /* [16], the problem's */;
  int n, m, ne, N, B;
  bool pm, dtb;           // DevProblem::pm / dtb are set
  const double* pm_host;  // [16, B] while pm: the handle's per-trajectory plants
  bool rollout_compiled, mc_compiled; int noise_mask;  // ModelOps: policy_rollout / policy_rollout_mc exist; policy_noise_mask
  int gains_pieces;       // ModelOps::gains_lds_pieces where the model stages gains through LDS, else 0
  const char* map_env; const char* chunk_env;  // TRAJOPT_POLICY_MAP / TRAJOPT_POLICY_CHUNK_WAVES as the environment has them (NULL: unset)
};
// noise == NULL (or nothing set in it) is to_policy_rollout itself, the NZ = 0 kernel and nothing else.  force_packed: the packed lane map
// whatever map_env says (to_mpc_advance: its S = 1 staging blocks must have the row layout of the nominal tiles, k_mpc.h).  Fills *run
// except the device pointers of run->pa (null); *plants: the [16, S, B] array to upload while run->nz has bit 2 (the caller's, or
// run->own_plants), else NULL.  A refused call leaves both untouched.
inline int lower_policy_opts(const PolicyFacts& f, int32_t S, const to_policy_opts* opts, const to_policy_noise* noise, bool force_packed, PolicyRun* run,
                             const double** plants) {
  if (S < 1) return fail(TO_ERR_ARGUMENT, "to_policy_rollout: S must be >= 1");
  if (!f.rollout_compiled) return fail(TO_ERR_UNSUPPORTED, "policy rollout not compiled for this model");
  to_policy_opts o = {1, 0, 0.0, nullptr, nullptr, nullptr};
  if (opts) o = *opts;
  if (o.refresh_gains != 0 && o.refresh_gains != 1) return fail(TO_ERR_ARGUMENT, "to_policy_rollout: refresh_gains must be 0 or 1");
  if (!std::isfinite(o.alpha)) return fail(TO_ERR_ARGUMENT, "to_policy_rollout: alpha must be finite");
  if (o.plant_params) if (int r = validate_plant_params("to_policy_rollout", f.model_key, f.mp, o.plant_params, false, "")) return r;
  const int m = f.m, B = f.B;
  PolicyRun R;
  PolicyArgs& pa = R.pa;
  std::memset(&pa, 0, sizeof(pa));
  int& nz = R.nz;
  if (noise) {
    if ((noise->sigma_w || noise->sigma_v) && (f.model_key == 7 || f.model_key == 8))
      return fail(TO_ERR_UNSUPPORTED, "to_policy_rollout_mc: sigma_w / sigma_v on a hybrid model or a model vector (their padded coordinates must stay "
                                      "exactly 0 and their live dimensions change per knot)");
    for (int kind = 0; kind < 2; ++kind) {
      const double* sg = kind == 0 ? noise->sigma_w : noise->sigma_v;
      if (!sg) continue;
      for (int i = 0; i < f.ne; ++i) {
        if (!std::isfinite(sg[i]) || sg[i] < 0.0)
          return fail(TO_ERR_ARGUMENT, std::string("to_policy_rollout_mc: ") + (kind == 0 ? "sigma_w" : "sigma_v") + " must be finite and >= 0");
        (kind == 0 ? pa.sigma_w : pa.sigma_v)[i] = sg[i];
      }
      nz |= 1 << kind;
    }
    if (noise->plant_params) {
      if (o.plant_params) return fail(TO_ERR_ARGUMENT, "to_policy_rollout_mc: plant_params given both in the options (one plant) and in the noise (one per sample)");
      for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s) {
          const double* pp = noise->plant_params + ((size_t)b * S + s) * 16;
          if (!plant_params_compatible(f.model_key, f.mp, pp))
            return validate_plant_params("to_policy_rollout", f.model_key, f.mp, pp, false, " of sample (b = " + std::to_string(b) + ", s = " + std::to_string(s) + ")");
        }
      nz |= 4;
    }
    pa.seed = noise->seed; pa.traj_offset = noise->traj_offset; pa.sample_offset = noise->sample_offset;
  }
  // A handle planned on one plant per trajectory (to_set_model_params_batch) simulates each trajectory on ITS plant when the caller names none:
  // the host fills the per-sample plants array and the one-plant-per-sample instance runs (an explicit plant, shared or per sample, overrides)
  const double* plants_src = (noise && noise->plant_params) ? noise->plant_params : nullptr;
  // (a handle with per-trajectory time steps, DevProblem::dtb, always takes a one-plant-per-sample instance — only those read the steps per
  // trajectory — so there an explicit shared plant is repeated for every sample)
  if (f.pm && !plants_src && (!o.plant_params || f.dtb)) {
    R.own_plants.resize((size_t)16 * S * B);
    for (int b = 0; b < B; ++b)
      for (int s = 0; s < S; ++s)
        std::memcpy(&R.own_plants[((size_t)b * S + s) * 16], o.plant_params ? o.plant_params : f.pm_host + (size_t)16 * b, sizeof(double) * 16);
    plants_src = R.own_plants.data();
    nz |= 4;
  }
  if (nz && (!f.mc_compiled || (nz & ~f.noise_mask))) return fail(TO_ERR_UNSUPPORTED, "to_policy_rollout_mc: not compiled for this model");
  // lane map, waves and every buffer length: path_plan.h plan_policy
  const PolicyPlan& pl = R.plan = plan_policy(f.n, m, f.N, B, S, force_packed ? nullptr : f.map_env, f.chunk_env, f.gains_pieces);
  R.packed = pl.packed;
  pa.S = S; pa.TPW = pl.TPW; pa.WPT = pl.WPT;
  if (pl.waves > 0x7fffffffLL / 64) return fail(TO_ERR_ARGUMENT, "to_policy_rollout: S * B is too large for one call");
  R.waves = (int)pl.waves;
  R.SB = pl.SB;
  pa.alpha = o.alpha;
  pa.clamp = (o.u_min || o.u_max) ? 1 : 0;
  for (int j = 0; j < TO_MAX_M; ++j) {
    pa.u_min[j] = (o.u_min && j < m) ? o.u_min[j] : -HUGE_VAL;
    pa.u_max[j] = (o.u_max && j < m) ? o.u_max[j] : HUGE_VAL;
    if (!(pa.u_min[j] <= pa.u_max[j])) return fail(TO_ERR_ARGUMENT, "to_policy_rollout: u_min must not exceed u_max");
  }
  std::memcpy(pa.mp, o.plant_params ? o.plant_params : f.mp, sizeof(pa.mp));
  R.refresh_gains = o.refresh_gains != 0;
  *run = std::move(R);  // (own_plants keeps its buffer: plants_src stays valid)
  *plants = plants_src;
  return TO_OK;
}

// to_mpc_opts (to_mpc_advance), in the order its refusals have always come, and MpcArgs::u_fill (k_mpc.h): the caller's control for j < m,
// zero beyond.  model_key / model_name as in MpcDualFacts.  A refused call leaves u_fill untouched.
struct MpcFacts {
  int model_key; const char* model_name;
  int N, m;
};
inline int lower_mpc_opts(const MpcFacts& f, const to_mpc_opts* mpc, double u_fill[TO_MAX_M]) {
  if (!mpc) return fail(TO_ERR_NULL, "to_mpc_advance: mpc is NULL");
  if (f.model_key >= 7)  // a shift changes which model governs a knot (hybrid, model vector); slack controls have no meaning once shifted
    return fail(TO_ERR_UNSUPPORTED, std::string("to_mpc_advance: not available for the ") + f.model_name +
                                        " (TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, TO_MODEL_VECTOR and TO_MODEL_INFEASIBLE cannot shift their plan)");
  if (mpc->shift < 1 || mpc->shift > f.N - 2)
    return fail(TO_ERR_ARGUMENT, "to_mpc_advance: shift must be in 1 .. N-2 = " + std::to_string(f.N - 2) + "; got " + std::to_string(mpc->shift));
  if (mpc->guess != TO_MPC_GUESS_CLOSED_LOOP && mpc->guess != TO_MPC_GUESS_NOMINAL)
    return fail(TO_ERR_ARGUMENT, "to_mpc_advance: guess must be TO_MPC_GUESS_CLOSED_LOOP (0) or TO_MPC_GUESS_NOMINAL (1)");
  if (mpc->tail != TO_MPC_TAIL_HOLD && mpc->tail != TO_MPC_TAIL_FILL)
    return fail(TO_ERR_ARGUMENT, "to_mpc_advance: tail must be TO_MPC_TAIL_HOLD (0) or TO_MPC_TAIL_FILL (1)");
  if (mpc->reserved != 0) return fail(TO_ERR_ARGUMENT, "to_mpc_advance: reserved must be 0");
  double fill[TO_MAX_M] = {};
  if (mpc->tail == TO_MPC_TAIL_FILL) {
    if (!mpc->u_fill) return fail(TO_ERR_NULL, "to_mpc_advance: TO_MPC_TAIL_FILL needs u_fill");
    for (int j = 0; j < f.m; ++j) {
      if (!std::isfinite(mpc->u_fill[j])) return fail(TO_ERR_ARGUMENT, "to_mpc_advance: u_fill must be finite");
      fill[j] = mpc->u_fill[j];
    }
  }
  std::memcpy(u_fill, fill, sizeof(fill));
  return TO_OK;
}

}  // namespace to
