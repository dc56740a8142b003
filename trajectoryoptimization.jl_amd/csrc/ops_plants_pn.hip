// ops_plants_pn.hip — one plant per trajectory (DevProblem::pm): the flagged instances of the projected-Newton polish and of the
// dynamics-defect kernel (k_pn.h PM), for the models to_set_model_params_batch accepts.
#include "ops_pn.h"

namespace to {
template <class M>
static void fill_one(ModelOps& o) { o.pn_launch[1] = op_pn_launch<M, true>; o.defect[1] = op_defect<M, true>; }

void fill_ops_plants_pn(ModelOps* t) {
  fill_one<DoubleIntegratorModel<1>>(t[0]);
  fill_one<DoubleIntegratorModel<2>>(t[1]);
  fill_one<DoubleIntegratorModel<3>>(t[2]);
  fill_one<CartpoleModel>(t[3]);
  fill_one<QuadrotorModel>(t[4]);
}
}  // namespace to
