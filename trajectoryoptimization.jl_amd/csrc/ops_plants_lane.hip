// ops_plants_lane.hip — one plant per trajectory (DevProblem::pm), small models on the lane layout: the flagged general instance of
// k_expand_lane, compiled with the flags of ops_small_lane.hip (build.py) so that its chunk-mode dual numbers fold the same zeros.
#include "ops_lane.h"

namespace to {
template <class M>
static void fill_one(ModelOps& o) {
  if constexpr (M::lane_backward && !M::lie) o.expand_lane_k[1] = op_expand_lane<M, true>;
}
void fill_ops_plants_lane(ModelOps* t) {
  fill_one<DoubleIntegratorModel<1>>(t[0]);
  fill_one<DoubleIntegratorModel<2>>(t[1]);
  fill_one<DoubleIntegratorModel<3>>(t[2]);
  fill_one<CartpoleModel>(t[3]);
}
}  // namespace to
