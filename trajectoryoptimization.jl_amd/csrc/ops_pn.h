// ops_pn.h — launchers of the projected-Newton kernels and the dynamics-defect kernel (k_pn.h), shared by ops_pn.hip and by the
// translation unit of their per-trajectory-plant instances (ops_plants_pn.hip: PM, DevProblem::pm).
#pragma once
#include "handle.h"
#include "k_pn.h"

namespace to {

template <class M, bool PM = false>
int op_pn_launch(to_handle* h, int slot0, int count, hipStream_t stream, const to_solver_opts* opts) {
  if (count <= 0) return TO_OK;
  const int N = h->a.P.N;
  PnArgs q;
  q.a = h->a;
  q.a.P.opts = *opts;
  q.pak = h->pn_pak; q.koff = h->pn_koff; q.list = h->pn_list; q.nbmax = h->pn_nbmax;
  q.ws = h->pn_ws + (size_t)slot0 * (size_t)h->pn_per;
  q.base = slot0;
  q.it_pn = h->a.it_pn; q.cmax_out = h->a.pn_cmax;
  const size_t lds = sizeof(double) * (size_t)pn_lds_doubles<M>(q.nbmax);
  constexpr int nc = M::ne + M::m;
  const int col_blocks = ((N - 1) * nc + 63) / 64, knot_blocks = N;
  return with_time_steps<M, PM>(h, [&](auto dt) {  // (DT: the flagged kernels on a handle with per-trajectory time steps, ops.h)
    constexpr bool DT = decltype(dt)::value;
    for (int round = 0; round <= opts->n_steps; ++round) {  // (n_steps >= 0: desc_lower.h) n_steps + 2 rounds, the last one its begin only
      enqueue(k_pn_begin<M, PM, DT>, dim3(count), dim3(64), lds, stream, q, round);
      enqueue(k_pn_lin_col<M, PM, DT>, dim3(count, col_blocks), dim3(64), 0, stream, q);
      with_weights<M>(h, [&](auto gw) { enqueue(k_pn_lin_knot<M, DT, decltype(gw)::value>, dim3(count, knot_blocks), dim3(64), 0, stream, q); return TO_OK; });
      enqueue(k_pn_project<M, PM, DT>, dim3(count), dim3(64), lds, stream, q);
    }
    return launch(k_pn_begin<M, PM, DT>, dim3(count), dim3(64), lds, stream, q, opts->n_steps + 1);
  });
}

template <class M, bool PM = false>
int op_defect(to_handle* h, double* out) {
  return with_time_steps<M, PM>(h, [&](auto dt) { return launch(k_defect<M, PM, decltype(dt)::value>, grid_b(h), dim3(BLOCK), 0, h->stream, h->a, out); });
}

}  // namespace to
