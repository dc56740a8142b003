// ops_lane.h — launchers of the one-lane-per-trajectory expansion kernels (k_expand_lane, k_expand_backward_lane).  Their
// translation units (ops_small_lane.hip; ops_hybrid.hip for the hybrid model) are the only ones that instantiate them:
// ops_small_lane.hip is compiled with -fno-honor-nans -fno-honor-infinities -fno-signed-zeros (build.py), which lets the compiler
// fold the structural zeros of chunk-mode dual numbers (x * 0.0, y + 0.0: IEEE forbids it otherwise — a third of the Cartpole
// expansion's FP64 instructions were products with a literal zero).
#pragma once
#include "ops.h"

namespace to {

// PM: one plant per trajectory (DevProblem::pm) — the general variant only, with the parameters loaded per lane (= trajectory)
template <class M, bool PM = false>
int op_expand_lane(to_handle* h) {
  if constexpr (M::lane_backward && !M::lie) {
    const dim3 lgrid(h->a.P.Bp / BLOCK, h->a.P.N);
    return with_integrator<M>(h, [&](auto fi) {
      return with_variant<!PM, CostWeightsModel<M>::value>(h, [&](auto v) {
        return with_time_steps<M, PM>(h, [&](auto dt) {
          return launch(k_expand_lane<M, decltype(fi)::value, decltype(v)::value, PM, decltype(dt)::value>, lgrid, dim3(BLOCK), 0, h->stream, h->a);
        });
      });
    });
  }
  return fail(TO_ERR_UNSUPPORTED, "lane expansion not compiled for this model");
}

// large batches of the small models: expansion fused into the one-lane-per-trajectory backward pass (k_expand.h)
template <class M>
int op_expand_backward(to_handle* h) {
  if constexpr (M::lane_backward && !M::lie) {
    const dim3 grid(h->a.P.Bp / BLOCK);
    return with_integrator<M>(h, [&](auto fi) {
      return with_variant<true, CostWeightsModel<M>::value>(h, [&](auto v) { return launch(k_expand_backward_lane<M, decltype(fi)::value, decltype(v)::value>, grid, dim3(BLOCK), 0, h->stream, h->a); });
    });
  }
  return fail(TO_ERR_UNSUPPORTED, "fused lane expansion + backward pass not compiled for this model");
}

}  // namespace to
