// ops_policy.hip — closed-loop policy rollouts (k_policy.h, to_policy_rollout) of every model family, both lane maps.
#include "ops.h"

namespace to {
void fill_ops_policy(ModelOps* t) {
  t[0].policy_rollout = op_policy_rollout<DoubleIntegratorModel<1>>;
  t[1].policy_rollout = op_policy_rollout<DoubleIntegratorModel<2>>;
  t[2].policy_rollout = op_policy_rollout<DoubleIntegratorModel<3>>;
  t[3].policy_rollout = op_policy_rollout<CartpoleModel>;
  t[4].policy_rollout = op_policy_rollout<QuadrotorModel>;
  t[5].policy_rollout = op_policy_rollout<QuadrotorAttModel<ATT_MRP>>;
  t[6].policy_rollout = op_policy_rollout<QuadrotorAttModel<ATT_RP>>;
  t[7].policy_rollout = op_policy_rollout<HybridDoubleIntegratorModel>;
  t[8].policy_rollout = op_policy_rollout<ModelVectorModel>;
  t[9].policy_rollout = op_policy_rollout<InfeasibleModel<DoubleIntegratorModel<1>>>;
  t[10].policy_rollout = op_policy_rollout<InfeasibleModel<DoubleIntegratorModel<2>>>;
  t[11].policy_rollout = op_policy_rollout<InfeasibleModel<CartpoleModel>>;
}
}  // namespace to
