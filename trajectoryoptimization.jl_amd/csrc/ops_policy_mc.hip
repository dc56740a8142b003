// ops_policy_mc.hip — the stochastic instances of the closed-loop policy rollout (k_policy.h with NZ != 0, to_policy_rollout_mc): process
// noise (bit 0), measurement noise (bit 1), one plant per sample (bit 2).  Every model with a fixed state layout gets all seven; the hybrid
// double integrator, whose padded coordinates must stay exactly 0, gets the per-sample plant only; a model vector takes no plant parameters
// at all and is served by the NZ = 0 kernel of ops_policy.hip.
#include "ops.h"

namespace to {

template <class M, bool NOISE>
int op_policy_rollout_mc(to_handle* h, const PolicyArgs& pa, int waves, int nz) {
  if (nz == 4) return op_policy_rollout<M, 4>(h, pa, waves);
  if constexpr (NOISE) {
    switch (nz) {
      case 1: return op_policy_rollout<M, 1>(h, pa, waves);
      case 2: return op_policy_rollout<M, 2>(h, pa, waves);
      case 3: return op_policy_rollout<M, 3>(h, pa, waves);
      case 5: return op_policy_rollout<M, 5>(h, pa, waves);
      case 6: return op_policy_rollout<M, 6>(h, pa, waves);
      case 7: return op_policy_rollout<M, 7>(h, pa, waves);
    }
  }
  return fail(TO_ERR_UNSUPPORTED, "policy rollout: no kernel instance for this combination of noise and plants on this model");
}

template <class M>
static void set_mc(ModelOps& t) {
  t.policy_rollout_mc = op_policy_rollout_mc<M, true>;
  t.policy_noise_mask = 7;
}

void fill_ops_policy_mc(ModelOps* t) {
  set_mc<DoubleIntegratorModel<1>>(t[0]);
  set_mc<DoubleIntegratorModel<2>>(t[1]);
  set_mc<DoubleIntegratorModel<3>>(t[2]);
  set_mc<CartpoleModel>(t[3]);
  set_mc<QuadrotorModel>(t[4]);
  set_mc<QuadrotorAttModel<ATT_MRP>>(t[5]);
  set_mc<QuadrotorAttModel<ATT_RP>>(t[6]);
  t[7].policy_rollout_mc = op_policy_rollout_mc<HybridDoubleIntegratorModel, false>;  // the per-sample plant only
  t[7].policy_noise_mask = 4;
  set_mc<InfeasibleModel<DoubleIntegratorModel<1>>>(t[9]);
  set_mc<InfeasibleModel<DoubleIntegratorModel<2>>>(t[10]);
  set_mc<InfeasibleModel<CartpoleModel>>(t[11]);
}
}  // namespace to
