// ops_plants_quad_forward.hip — one plant per trajectory (DevProblem::pm), quaternion Quadrotor: the general forward-pass variants with
// the plant loaded per trajectory (k_forward.h MODE bits 3 and 5), without and with constraints.
#include "ops.h"

namespace to {
void fill_ops_plants_quad_forward(ModelOps* t) {
  fill_forward_pm<QuadrotorModel, 8>(t[4]);
  fill_forward_pm<QuadrotorModel, 10>(t[4]);
}
}  // namespace to
