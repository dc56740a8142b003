// ops_infeasible_b.hip — Altro's InfeasibleModel over the Cartpole (see ops_infeasible_a.hip).
#include "ops.h"

namespace to {
void fill_ops_infeasible_b(ModelOps* t) {
  using M = InfeasibleModel<CartpoleModel>;
  fill_misc<M>(t[11]);
  t[11].expand[0] = op_expand<M>;
  t[11].backward = op_backward<M>;
  t[11].accept_roll = op_accept_roll<M>;
  t[11].infeasible_controls = op_infeasible_controls<M>;
  fill_forward<M, 0, 16>(t[11]);
  fill_forward2<M, 0, 16>(t[11]);
}
}  // namespace to
