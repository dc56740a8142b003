// ops_plants_quad.hip — one plant per trajectory (DevProblem::pm), quaternion Quadrotor: the flagged instances of the rollout, the
// dynamics Jacobian and the general expansion on the full tangent-matrix layout (compiled with the flags of ops_quad_expand.hip).
#include "ops.h"

namespace to {
void fill_ops_plants_quad(ModelOps* t) {
  t[4].rollout[1] = op_rollout<QuadrotorModel, true>;
  t[4].discrete_jacobian[1] = op_discrete_jacobian<QuadrotorModel, true>;
  t[4].expand[1] = op_expand_pm<QuadrotorModel>;
}
}  // namespace to
