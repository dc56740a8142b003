// ops_plants_quad.hip — one plant per trajectory (DevProblem::pm), quaternion Quadrotor: the flagged instances of the rollout, the
// dynamics Jacobian and the general expansion on the full tangent-matrix layout (compiled with the flags of ops_quad_expand.hip).
#include "ops.h"

namespace to {
void fill_ops_plants_quad(ModelOps* t) {
  t[4].rollout_pm = op_rollout_pm<QuadrotorModel>;
  t[4].discrete_jacobian_pm = op_discrete_jacobian_pm<QuadrotorModel>;
  t[4].expand_pm = op_expand_pm<QuadrotorModel>;
}
}  // namespace to
