// ops_plants_forward.hip — one plant per trajectory (DevProblem::pm), small models: the general forward-pass variants (k_forward.h MODE
// bit 3) with the plant loaded per trajectory (bit 5); one-wave workgroups, -ffp-contract=on like every forward translation unit.
#include "ops.h"

namespace to {
template <class M>
static void fill_one(ModelOps& o) {
  fill_forward_pm<M, 8>(o); fill_forward_pm<M, 10>(o); fill_forward_pm<M, 12>(o); fill_forward_pm<M, 14>(o);
}
void fill_ops_plants_forward(ModelOps* t) {
  fill_one<DoubleIntegratorModel<1>>(t[0]);
  fill_one<DoubleIntegratorModel<2>>(t[1]);
  fill_one<DoubleIntegratorModel<3>>(t[2]);
  fill_one<CartpoleModel>(t[3]);
}
}  // namespace to
