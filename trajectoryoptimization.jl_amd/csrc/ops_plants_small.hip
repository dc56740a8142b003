// ops_plants_small.hip — one plant per trajectory (DevProblem::pm, to_set_model_params_batch), small models: the flagged instances of the
// rollout, the dynamics Jacobian and the general expansion on the column / tangent-matrix layouts.
#include "ops.h"

namespace to {
template <class M>
static void fill_one(ModelOps& o) {
  o.rollout[1] = op_rollout<M, true>;
  o.discrete_jacobian[1] = op_discrete_jacobian<M, true>;
  o.expand[1] = op_expand_pm<M>;
}
void fill_ops_plants_small(ModelOps* t) {
  fill_one<DoubleIntegratorModel<1>>(t[0]);
  fill_one<DoubleIntegratorModel<2>>(t[1]);
  fill_one<DoubleIntegratorModel<3>>(t[2]);
  fill_one<CartpoleModel>(t[3]);
}
}  // namespace to
