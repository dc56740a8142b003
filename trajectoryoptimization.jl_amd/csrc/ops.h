// ops.h — launchers of the model-templated kernels; instantiated per model by the ops_*.hip translation units.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "handle.h"
#include "k_backward.h"
#include "k_expand.h"
#include "k_forward.h"
#include "k_scan.h"
#include "k_misc.h"
#include "k_policy.h"

namespace to {

template <class M>
void fill_traits(ModelOps& o) {
  o.write_through = M::accept_write_through;
  o.mfma_backward = M::mfma_backward;
  o.coop_backward = M::coop_backward;
  o.lane_backward = M::lane_backward;
  o.lds_gains = M::lds_gains;
  o.expand_knots = M::expand_knots;
  o.ls_first_round = M::ls_first_round;
  o.gains_lds_pieces = Gains<M>::RSK / 2;
  if constexpr (M::mfma_backward) {  // tangent-matrix layout traits (one 16 x 16 tile per knot: models with m <= 4)
    o.nep = Tm<M>::NEP; o.rs = Tm<M>::RS;
    for (int g = 0; g < 4; ++g)
      for (int c = 0; c < 16; ++c) o.crow[g * 16 + c] = compact_row<M>(g, c);
  }
}

// THE compile-time RK4 pin: body(fi) with fi = std::integral_constant<int, INTEG_RK4> when the model pins RK4 (M::pin_rk4) and the handle
// integrates with it, else <int, -1> (the integrator read at run time) — the FIXED_INTEG argument of the kernels that integrate.
template <class M, class F>
int with_integrator(const to_handle* h, F&& body) {
  if constexpr (M::pin_rk4) {
    if (h->a.P.integrator == INTEG_RK4) return body(std::integral_constant<int, INTEG_RK4>{});
  }
  return body(std::integral_constant<int, -1>{});
}
// THE expansion-variant ladder: body(v) with v = std::integral_constant<int, VAR> of the handle's problem — 0 = diagonal-kind costs, no
// constraints; 2 = + selector / SOC-selector constraints; 7 = everything; 15 = everything, with the diagonal weights of the costs read per
// trajectory (DevProblem::gw set: bit 3, k_expand.h; WEIGHTS = false, the models the setter refuses: no such instance).  SPECIAL = false: the
// general variants only (the flagged instances of one plant per trajectory).  A body that has no instance of a variant guards it with `if constexpr`.
template <bool SPECIAL = true, bool WEIGHTS = true, class F>
int with_variant(const to_handle* h, F&& body) {
  if constexpr (SPECIAL) {
    if (h->a.P.expand_variant == 0) return body(std::integral_constant<int, 0>{});
    if (h->a.P.expand_variant == 2) return body(std::integral_constant<int, 2>{});
  }
  if constexpr (WEIGHTS) {
    if (h->a.P.gw != nullptr) return body(std::integral_constant<int, 15>{});
  }
  return body(std::integral_constant<int, 7>{});
}

// (PM, here and below: the flagged instance that loads one plant per trajectory, DevProblem::pm — instantiated by the ops_plants_*.hip units)
template <class M, bool PM = false>
int op_rollout(to_handle* h) {
  return with_integrator<M>(h, [&](auto fi) {
    return with_time_steps<M, PM>(h, [&](auto dt) { return launch(k_rollout<M, decltype(fi)::value, PM, decltype(dt)::value>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a); });
  });
}
template <class M>
int op_cost(to_handle* h, int with_al, double* out, double* Jk) {
  return with_weights<M>(h, [&](auto gw) { return launch(k_cost<M, decltype(gw)::value>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a, with_al, out, Jk); });
}
template <class M>
int op_violation(to_handle* h, double* out) {
  return launch(k_violation<M>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a, out);
}
template <class M>
int op_dual_update(to_handle* h) {
  return launch(k_dual_update<M>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a);
}
// AL outer update of the trajectories whose inner solve ended in this batch step (k_misc.h, k_outer_*)
template <class M>
int op_outer(to_handle* h) {
  const int N = h->a.P.N;
  enqueue(k_outer_violation<M>, grid_b(h, N), dim3(BLOCK), 0, h->stream, h->a);
  enqueue(k_outer_decide<M>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a);
  with_weights<M>(h, [&](auto gw) { enqueue(k_outer_update<M, decltype(gw)::value>, grid_b(h, N), dim3(BLOCK), 0, h->stream, h->a); return TO_OK; });
  return launch(k_outer_finish<M>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a);
}
template <class M>
int op_cost_derivs(to_handle* h, double* dg, double* dh) {
  return with_weights<M>(h, [&](auto gw) { return launch(k_cost_derivs<M, decltype(gw)::value>, grid_b(h, h->a.P.N), dim3(BLOCK), 0, h->stream, h->a, dg, dh); });
}
template <class M, bool PM = false>
int op_discrete_jacobian(to_handle* h, double* F) {
  const DevProblem& P = h->a.P;
  return with_time_steps<M, PM>(h, [&](auto dt) { return launch(k_discrete_jacobian<M, PM, decltype(dt)::value>, grid_b(h, P.N - 1, P.n + P.m), dim3(BLOCK), 0, h->stream, h->a, F); });
}
template <class M>
int op_constraint_eval(to_handle* h, int ci, double* vals, double* jac) {
  const DevCon& c = h->cons[ci];
  return launch(k_constraint_eval<M>, grid_b(h, c.k2 - c.k1 + 1), dim3(BLOCK), 0, h->stream, h->a, ci, vals, jac);
}
template <class M>
int op_constraint_hessian(to_handle* h, int ci, const double* lambda, double* H) {
  const DevCon& c = h->cons[ci];
  return launch(k_constraint_hessian<M>, grid_b(h, c.k2 - c.k1 + 1), dim3(BLOCK), 0, h->stream, h->a, ci, lambda, H);
}
template <class M>
int op_infeasible_controls(to_handle* h) {  // InfeasibleModel only
  return launch(k_infeasible_controls<M>, grid_b(h, h->a.P.N - 1), dim3(BLOCK), 0, h->stream, h->a);
}

// Expansion, in the variant (with_variant) and the layout (k_expand.h LAY) of the handle: column layout (0) for the cooperative backward pass,
// tangent-matrix layout with the full (1) or the compact (2: variants 0 and 2 only) cost block for the MFMA one, lane layout (3) for the
// one-lane-per-trajectory one.
template <class M>
int op_expand(to_handle* h) {
  const DevProblem& P = h->a.P;
  const int lay = h->a.bwd_lane ? 3 : !h->a.bwd_mfma ? 0 : (h->a.h_compact ? 2 : 1);
  // lane layout: one lane per (trajectory, knot), all columns at once (k_expand_lane; instantiated in the lane translation units, ops_lane.h)
  if (lay == 3 && h->plan.expand_lane && h->ops->expand_lane_k[0]) return h->ops->expand_lane_k[0](h);
  return with_integrator<M>(h, [&](auto fi) {
    return with_variant<true, CostWeightsModel<M>::value>(h, [&](auto v) {
      constexpr int FI = decltype(fi)::value, V = decltype(v)::value;
      constexpr int kc = expand_kc<M, V == 0 ? 0 : 2>();
      const dim3 grid((P.B + h->G - 1) / h->G, (P.N + kc - 1) / kc);
      if constexpr (M::mfma_backward && ExpandPack<M>::ok && (V & 4) == 0) {  // compact cost block of the quaternion rigid body: the packed expansion (k_expand.h)
        if (lay == 2 && h->plan.expand_pack)
          return launch(k_expand<M, FI, V, 2, true>, dim3((P.B + EXPAND_PACK_G - 1) / EXPAND_PACK_G, (P.N + kc - 1) / kc), dim3(BLOCK), 0, h->stream, h->a);
      }
      if constexpr (M::mfma_backward) {
        if (lay == 1) return launch(k_expand<M, FI, V, 1>, grid, dim3(BLOCK), 0, h->stream, h->a);
        if constexpr ((V & 4) == 0) {
          if (lay == 2) return launch(k_expand<M, FI, V, 2>, grid, dim3(BLOCK), 0, h->stream, h->a);
        }
      }
      if constexpr (!M::mfma_backward || M::coop_backward) {
        if (lay == 0) return launch(k_expand<M, FI, V, 0>, grid, dim3(BLOCK), 0, h->stream, h->a);
      }
      if constexpr (M::lane_backward) {
        if (lay == 3) return launch(k_expand<M, FI, V, 3>, grid, dim3(BLOCK), 0, h->stream, h->a);
      }
      return fail(TO_ERR_UNSUPPORTED, "expansion variant not compiled for this model");
    });
  });
}
// one plant per trajectory: the general variant (7) on the column layout or the full tangent-matrix layout (the handle's expand_variant has
// bit 2 forced: no compact cost block)
template <class M>
int op_expand_pm(to_handle* h) {
  const DevProblem& P = h->a.P;
  constexpr int kc = expand_kc<M, 2>();
  const dim3 grid((P.B + h->G - 1) / h->G, (P.N + kc - 1) / kc);
  if (h->a.bwd_lane || h->a.h_compact) return fail(TO_ERR_UNSUPPORTED, "per-trajectory model parameters: expansion layout without a flagged instance");
  return with_integrator<M>(h, [&](auto fi) {
    return with_variant<false, CostWeightsModel<M>::value>(h, [&](auto v) {  // (7, or 15 with per-trajectory cost weights)
      return with_time_steps<M, true>(h, [&](auto dt) {
        constexpr int FI = decltype(fi)::value, V = decltype(v)::value;
        constexpr bool DT = decltype(dt)::value;
        if constexpr (M::mfma_backward) {
          if (h->a.bwd_mfma) return launch(k_expand<M, FI, V, 1, false, true, DT>, grid, dim3(BLOCK), 0, h->stream, h->a);
        }
        if constexpr (!M::mfma_backward || M::coop_backward) {
          if (!h->a.bwd_mfma) return launch(k_expand<M, FI, V, 0, false, true, DT>, grid, dim3(BLOCK), 0, h->stream, h->a);
        }
        return fail(TO_ERR_UNSUPPORTED, "per-trajectory model parameters: expansion not compiled for this model and layout");
      });
    });
  });
}
template <class M>
int op_expand_const(to_handle* h) {
  const DevProblem& P = h->a.P;
  return launch(k_expand_const_columns<M>, dim3(P.B, (P.N - 1 + 3) / 4), dim3(BLOCK), 0, h->stream, h->a);
}
template <class M>
int op_backward(to_handle* h) {
  const DevProblem& P = h->a.P;
  if constexpr (M::mfma_backward) {
    if (h->a.bwd_mfma) {
      if (h->a.h_compact) return launch(k_backward_mfma<M, true>, dim3(P.B), dim3(BLOCK), 0, h->stream, h->a);
      return launch(k_backward_mfma<M, false>, dim3(P.B), dim3(BLOCK), 0, h->stream, h->a);
    }
  }
  if constexpr (M::lane_backward) {
    if (h->a.bwd_lane) return launch(k_backward_lane<M>, dim3((P.B + 63) / 64), dim3(BLOCK), 0, h->stream, h->a);
  }
  if constexpr (!M::mfma_backward || M::coop_backward) {
    if (h->a.h_diag) return launch(k_backward_coop<M, true>, dim3((P.B + h->G - 1) / h->G), dim3(BLOCK), 0, h->stream, h->a);
    return launch(k_backward_coop<M, false>, dim3((P.B + h->G - 1) / h->G), dim3(BLOCK), 0, h->stream, h->a);
  }
  return fail(TO_ERR_UNSUPPORTED, "backward-pass variant not compiled for this model");
}

// small batches of the small models with diagonal cost blocks (variants 0 and 2): expansion fused into the cooperative backward pass (k_expand.h)
template <class M>
int op_expand_backward_coop(to_handle* h) {
  if constexpr (!M::lie && Coop<M>::R <= 8 && (!M::mfma_backward || M::coop_backward)) {
    const dim3 grid((h->a.P.B + h->G - 1) / h->G);
    return with_integrator<M>(h, [&](auto fi) {
      return with_variant(h, [&](auto v) {
        constexpr int FI = decltype(fi)::value, V = decltype(v)::value;
        if constexpr ((V & 4) == 0) {
          if (h->a.coop_merge != 0) return launch(k_expand_backward_coop<M, FI, V, true>, grid, dim3(128), 0, h->stream, h->a);
          return launch(k_expand_backward_coop<M, FI, V, false>, grid, dim3(128), 0, h->stream, h->a);
        }
        return fail(TO_ERR_UNSUPPORTED, "fused cooperative pass needs diagonal cost blocks");
      });
    });
  }
  return fail(TO_ERR_UNSUPPORTED, "fused expansion + cooperative backward pass not compiled for this model");
}

// fused expansion + scan backward pass (k_scan.h): unconstrained problems with diagonal cost blocks, one wave per trajectory
template <class M>
int op_expand_backward_scan(to_handle* h) {
  if constexpr (!M::lie && M::ne <= 4 && M::m <= 2) {
    const DevProblem& P = h->a.P;
    if (P.expand_variant != 0 || !h->a.h_diag || P.N > 126) return fail(TO_ERR_UNSUPPORTED, "scan backward pass: outside its scope");
    // TRAJOPT_SCAN_TRIM=0: the untrimmed round loop (a testing switch read at the launch, so that one process can compare the two
    // instances; results do not depend on it)
    const char* env = std::getenv("TRAJOPT_SCAN_TRIM");
    const bool trim = !(env && std::atoi(env) == 0);
    return with_integrator<M>(h, [&](auto fi) {
      constexpr int FI = decltype(fi)::value;
      if (!trim) return launch(k_expand_backward_scan<M, FI, 0, false>, dim3(P.B), dim3(64), 0, h->stream, h->a);
      return launch(k_expand_backward_scan<M, FI, 0, true>, dim3(P.B), dim3(64), 0, h->stream, h->a);
    });
  }
  return fail(TO_ERR_UNSUPPORTED, "scan backward pass not compiled for this model");
}

// forward pass (line search + state machine) of kernel variant MODE: grid = one wave per TW = 64 / CW trajectories
template <class M, int MODE>
int op_forward(to_handle* h) {
  const KArgs& a = h->a;
  const int TW = a.TW;
  const size_t lds = M::lds_gains ? sizeof(double) * (2 * gains_lds_doubles<M>(TW) + StageCostLds<M::n, M::m>::size) : 0;  // two gains buffers + the stage-cost table
  // (the flagged variants, bit 5, with per-trajectory time steps: bit 6)
  return with_time_steps<M, (MODE & 32) != 0>(h, [&](auto dt) {
    return launch(k_forward<M, (MODE | (decltype(dt)::value ? 64 : 0))>, dim3((a.P.Bp + TW - 1) / TW), dim3(BLOCK), lds, h->stream, a);
  });
}

// accepted steps re-rolled from their stored controls (k_accept_roll; models without write-through)
template <class M>
int op_accept_roll(to_handle* h) {
  enqueue(k_accept_gather_u<M>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a);
  return with_integrator<M>(h, [&](auto fi) { return launch(k_accept_roll<M, decltype(fi)::value>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a); });
}

// closed-loop policy rollout (k_policy.h), NZ = 0 or one of its stochastic instances (ops_policy_mc.hip): pa.TPW == 0 selects the uniform
// lane map; grid = the waves of this launch
template <class M, int NZ = 0>
int op_policy_rollout(to_handle* h, const PolicyArgs& pa, int waves) {
  const bool uniform = pa.TPW == 0;
  const size_t lds = policy_lds_bytes(M::lds_gains ? Gains<M>::RSK / 2 : 0, uniform ? 1 : pa.TPW);  // two gains buffers (path_plan.h)
  static_assert(!M::lds_gains || Gains<M>::RSK % 2 == 0, "gains rows must be whole 16-byte pieces");
  return with_integrator<M>(h, [&](auto fi) {
    return with_time_steps<M, (NZ & 4) != 0>(h, [&](auto dt) {  // (a handle with per-trajectory time steps runs a one-plant-per-sample instance)
      return with_weights<M>(h, [&](auto gw) {  // (... and one with per-trajectory cost weights the instance that reads them for J)
        constexpr int FI = decltype(fi)::value;
        constexpr bool DT = decltype(dt)::value, GW = decltype(gw)::value;
        if (uniform) return launch(k_policy_rollout<M, true, FI, NZ, DT, GW>, dim3(waves), dim3(BLOCK), lds, h->stream, h->a, pa);
        return launch(k_policy_rollout<M, false, FI, NZ, DT, GW>, dim3(waves), dim3(BLOCK), lds, h->stream, h->a, pa);
      });
    });
  });
}

template <class M, int MODE>
int op_forward2(to_handle* h) {
  const KArgs& a = h->a;
  const int TW = a.TW;
  // list mode: workgroups for the trajectories still active only (the host's count lags and only ever over-counts; the kernel reads the exact one)
  const int groups = a.fwd_list ? fwd_list_groups(h->list_active, TW) : (a.P.Bp + TW - 1) / TW;
  return launch(k_forward2<M, MODE>, dim3(groups), dim3(128), sizeof(double) * fwd2_lds_doubles<M>(TW), h->stream, a);
}
template <class M, int LO, int HI>
void fill_forward2(ModelOps& o) {
  if constexpr (LO < HI) {
    if constexpr (M::pin_rk4 || (LO & 4) == 0) o.forward2[LO] = op_forward2<M, LO>;
    fill_forward2<M, LO + 1, HI>(o);
  }
}
// one plant per trajectory: the general forward variants GEN (bit 3 set) with the plant loaded per trajectory (k_forward.h MODE bit 5)
template <class M, int GEN>
void fill_forward_pm(ModelOps& o) {
  static_assert((GEN & 8) != 0 && GEN < 32, "per-trajectory model parameters: general forward variants only");
  if constexpr (M::pin_rk4 || (GEN & 4) == 0) o.forward[1][GEN] = op_forward<M, (GEN | 32)>;
}

template <class M>
void fill_misc(ModelOps& o) {
  fill_traits<M>(o);
  o.rollout[0] = op_rollout<M>; o.cost = op_cost<M>; o.violation = op_violation<M>; o.dual_update = op_dual_update<M>;
  o.outer = op_outer<M>; o.cost_derivs = op_cost_derivs<M>; o.discrete_jacobian[0] = op_discrete_jacobian<M>;
  o.constraint_eval = op_constraint_eval<M>; o.constraint_hessian = op_constraint_hessian<M>;
}
// forward variants [LO, HI): models that do not pin RK4 never run the bit-2 variants
template <class M, int LO, int HI>
void fill_forward(ModelOps& o) {
  if constexpr (LO < HI) {
    if constexpr (M::pin_rk4 || (LO & 4) == 0) o.forward[0][LO] = op_forward<M, LO>;
    fill_forward<M, LO + 1, HI>(o);
  }
}

}  // namespace to
