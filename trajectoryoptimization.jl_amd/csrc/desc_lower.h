// desc_lower.h — host-side lowering of the C-ABI descriptors (include/trajopt_hip.h): solver-option defaults and validation,
// model dimensions, constraint descriptors -> DevCon (selector tables), cost validation, the whole problem (lower_problem: to_create), and the
// host half of every per-trajectory setter.  Pure host C++ (no HIP calls): shared
// by the library (trajopt_hip.hip) and by the host build of the projected-Newton kernel that the CPU test-suite runs
// (tests/host_shim/pn_harness.cpp).  Mirrors the reference's constructors: Problem src/problem.jl:44-72, add_constraint!
// src/constraint_list.jl:103-134, BoundConstraint src/constraints.jl:660-687, NormConstraint :442-455.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "models.h"
#include "problem_dev.h"

namespace to {
int fail(int code, const std::string& msg);  // records the message for to_last_error(), returns code

inline void default_opts(to_solver_opts* o) {
  std::memset(o, 0, sizeof(*o));
  o->cost_tolerance = 1e-4; o->gradient_tolerance = 10.0; o->iterations = 300; o->dJ_counter_limit = 10;
  o->iterations_linesearch = 20; o->line_search_lower_bound = 1e-8; o->line_search_upper_bound = 10.0;
  o->line_search_decrease_factor = 0.5; o->bp_reg_initial = 0.0; o->bp_reg_increase_factor = 1.6;
  o->bp_reg_min = 1e-8; o->bp_reg_max = 1e8; o->bp_reg_fp = 10.0; o->max_cost_value = 1e8;
  o->max_state_value = 1e8; o->max_control_value = 1e8; o->constraint_tolerance = 1e-6;
  o->cost_tolerance_intermediate = 1e-4; o->penalty_initial = 1.0; o->penalty_scaling = 10.0;
  o->penalty_max = 1e8; o->dual_max = 1e8; o->iterations_outer = 30; o->cost_dt_scaling = 0;
  o->iterations_total = 1000;
  o->projected_newton_tolerance = 1e-3; o->active_set_tolerance_pn = 1e-3; o->rho_chol = 1e-8; o->rho_primal = 1e-8;
  o->r_threshold = 1.1; o->n_steps = 2; o->projected_newton = 1;
}

// Nonsense options used to give silent non-termination-style behaviour (every trajectory runs to MAX_ITERATIONS).
inline int validate_opts(const to_solver_opts& o) {
  auto bad = [](const char* what) { return fail(TO_ERR_ARGUMENT, std::string("solver option out of range: ") + what); };
  if (!(o.cost_tolerance >= 0) || !(o.cost_tolerance_intermediate >= 0) || !(o.gradient_tolerance >= 0) || !(o.constraint_tolerance >= 0))
    return bad("tolerances must be >= 0");
  if (o.iterations < 0 || o.iterations_outer < 0 || o.iterations_total < 0 || o.dJ_counter_limit < 0) return bad("iteration counts must be >= 0");
  if (o.iterations_linesearch < 1 || o.iterations_linesearch > 64) return bad("iterations_linesearch must be in 1..64");
  if (!(o.line_search_decrease_factor > 0.0 && o.line_search_decrease_factor < 1.0)) return bad("line_search_decrease_factor must be in (0,1)");
  if (!(o.line_search_lower_bound >= 0.0) || !(o.line_search_upper_bound > o.line_search_lower_bound)) return bad("line-search bounds must satisfy 0 <= lower < upper");
  if (!(o.bp_reg_increase_factor > 1.0)) return bad("bp_reg_increase_factor must be > 1");
  if (!(o.bp_reg_initial >= 0.0) || !(o.bp_reg_min >= 0.0) || !(o.bp_reg_max > o.bp_reg_min) || !(o.bp_reg_fp >= 0.0)) return bad("regularisation bounds");
  if (!(o.penalty_initial > 0.0) || !(o.penalty_scaling >= 1.0) || !(o.penalty_max >= o.penalty_initial) || !(o.dual_max > 0.0)) return bad("penalty parameters");
  if (!(o.max_cost_value > 0.0) || !(o.max_state_value > 0.0) || !(o.max_control_value > 0.0)) return bad("max_*_value must be > 0");
  if (o.cost_dt_scaling != 0 && o.cost_dt_scaling != 1) return bad("cost_dt_scaling must be 0 or 1");
  if (o.al_full_newton != 0 && o.al_full_newton != 1) return bad("al_full_newton must be 0 or 1");
  if (!(o.projected_newton_tolerance >= 0) || !(o.active_set_tolerance_pn >= 0)) return bad("projected-Newton tolerances must be >= 0");
  if (!(o.rho_chol >= 0) || !(o.rho_primal > 0) || !(o.r_threshold > 0)) return bad("rho_chol >= 0, rho_primal > 0, r_threshold > 0");
  if (o.n_steps < 0 || (o.projected_newton != 0 && o.projected_newton != 1)) return bad("n_steps must be >= 0, projected_newton 0 or 1");
  return TO_OK;
}

inline int model_dims(int id, const double* params, int* n, int* m, int* ne, int* key) {
  switch (id) {
    case TO_MODEL_DOUBLE_INTEGRATOR: {
      const int D = (int)params[1];
      if (D < 1 || D > 3) return -1;
      *n = 2 * D; *m = D; *ne = 2 * D; *key = D - 1; return 0;
    }
    case TO_MODEL_CARTPOLE: *n = 4; *m = 1; *ne = 4; *key = 3; return 0;
    case TO_MODEL_QUADROTOR: {  // params[10]: attitude representation of the state (to_rotation)
      const int rot = (int)params[10];
      if (rot == TO_ROT_QUATERNION) { *n = 13; *m = 4; *ne = 12; *key = 4; return 0; }
      if (rot == TO_ROT_MRP || rot == TO_ROT_RODRIGUES) { *n = 12; *m = 4; *ne = 12; *key = rot == TO_ROT_MRP ? 5 : 6; return 0; }
      return -1;
    }
    case TO_MODEL_HYBRID_DOUBLE_INTEGRATOR: *n = 4; *m = 2; *ne = 4; *key = 7; return 0;
    case TO_MODEL_VECTOR: *n = TO_VECTOR_N; *m = TO_VECTOR_M; *ne = TO_VECTOR_N; *key = 8; return 0;
    case TO_MODEL_INFEASIBLE: {  // Altro's InfeasibleModel over a small vector-space base (models.h InfeasibleModel): params[15] = base id
      const int base = (int)params[15];
      if (base == TO_MODEL_DOUBLE_INTEGRATOR) {
        const int D = (int)params[1];
        if (D < 1 || D > 2) return -1;  // (D = 3: m = 3 + 6 exceeds TO_MAX_M)
        *n = 2 * D; *m = 3 * D; *ne = 2 * D; *key = 8 + D; return 0;
      }
      if (base == TO_MODEL_CARTPOLE) { *n = 4; *m = 5; *ne = 4; *key = 11; return 0; }
      return -1;
    }
  }
  return -1;
}

// Model vector (TO_MODEL_VECTOR): every check RD.dims(models) makes (src/dynamics.jl:15-31), and the per-step table the kernels
// read (models.h ModelVectorModel: 64 doubles per step).
inline int lower_step_models(const to_step_model* sm, int N, std::vector<double>* table) {
  if (!sm) return fail(TO_ERR_NULL, "TO_MODEL_VECTOR needs step_models[N-1]");
  table->assign((size_t)64 * (N - 1), 0.0);
  for (int k = 0; k < N - 1; ++k) {
    const to_step_model& s = sm[k];
    double* r = table->data() + (size_t)64 * k;
    if (s.n < 1 || s.n > TO_VECTOR_N || s.m < 1 || s.m > TO_VECTOR_M || s.n_out < 1 || s.n_out > TO_VECTOR_N)
      return fail(TO_ERR_UNSUPPORTED, "model vector: step dimensions outside (6, 3)");
    switch (s.kind) {
      case TO_STEP_DOUBLE_INTEGRATOR:
        if (s.n != 2 * s.m || s.n_out != s.n) return fail(TO_ERR_DIMENSION_MISMATCH, "double integrator step: n = 2D, m = D, n_out = n");
        if (!(s.params[0] > 0.0)) return fail(TO_ERR_ARGUMENT, "double integrator step: mass must be positive");
        r[4] = s.params[0]; r[5] = s.m;
        break;
      case TO_STEP_CARTPOLE:
        if (s.n != 4 || s.m != 1 || s.n_out != 4) return fail(TO_ERR_DIMENSION_MISMATCH, "Cartpole step: (n, m, n_out) = (4, 1, 4)");
        for (int i = 0; i < 4; ++i) r[4 + i] = s.params[i];
        break;
      case TO_STEP_LINEAR_MAP:
        for (int i = 0; i < s.n_out; ++i) {
          for (int j = 0; j < s.n; ++j) r[8 + 6 * i + j] = s.params[i + s.n_out * j];
          for (int j = 0; j < s.m; ++j) r[44 + 3 * i + j] = s.params[s.n_out * s.n + i + s.n_out * j];
        }
        break;
      default: return fail(TO_ERR_UNSUPPORTED, "unknown step model kind");
    }
    r[0] = s.kind; r[1] = s.n; r[2] = s.m; r[3] = s.n_out;
    if (k + 1 < N - 1 && sm[k + 1].n != s.n_out)  // RD.dims: "Model mismatch at time step k"
      return fail(TO_ERR_DIMENSION_MISMATCH, "Model mismatch at time step " + std::to_string(k + 1) + ". Model " + std::to_string(k + 1) +
                                                 " has an output dimension of " + std::to_string(s.n_out) + " but model " + std::to_string(k + 2) +
                                                 " has a state dimension of " + std::to_string(sm[k + 1].n) + ".");
  }
  return TO_OK;
}

inline int validate_constraint(int n, int m, int N, const to_constraint_desc& d, DevCon* out) {
  const int nz = n + m;
  DevCon ci;
  std::memset(&ci, 0, sizeof(ci));
  ci.d = d;
  ci.cp_off = -1;  // shared parameters (to_set_constraint_params_batch flags a constraint later)
  ci.cl_off = -1;  // shared limits (to_set_constraint_limits_batch)
  if (d.k_first < 1 || d.k_last > N || d.k_first > d.k_last)
    return fail(TO_ERR_ASSERTION, "Invalid inds, inds[end] must be less than number of knotpoints");  // src/constraint_list.jl:112
  if (d.n_inds < 0 || d.n_inds > TO_MAX_CON_INDS || d.n_params < 0 || d.n_params > TO_MAX_CON_PARAMS)
    return fail(TO_ERR_ARGUMENT, "constraint inds/params count out of range");
  auto dimerr = [&](const char* what) {
    return fail(TO_ERR_DIMENSION_MISMATCH, std::string("New constraint not consistent with n=") + std::to_string(n) +
                                               " and m=" + std::to_string(m) + ": " + what);  // src/constraint_list.jl:109
  };
  // index lists address [x;u] positions one-to-one: a duplicate would make the reported Jacobian (last duplicate wins)
  // disagree with the one the solver accumulates
  for (int i = 0; i < d.n_inds; ++i)
    for (int j = i + 1; j < d.n_inds; ++j)
      if (d.inds[i] == d.inds[j]) return fail(TO_ERR_ARGUMENT, "constraint indices must be distinct");
  int p = 0;
  switch (d.kind) {
    case TO_CON_GOAL:
      if (d.sense != TO_CONE_ZERO) return fail(TO_ERR_ARGUMENT, "GoalConstraint sense must be Equality");
      if (d.n_params != d.n_inds) return dimerr("GoalConstraint length(xf) != length(inds)");
      for (int i = 0; i < d.n_inds; ++i) if (d.inds[i] < 1 || d.inds[i] > n) return dimerr("GoalConstraint index outside the state");
      ci.width = n; p = d.n_inds; ci.selector = 1;
      for (int r = 0; r < p && r < TO_MAX_P; ++r) { ci.sidx[r] = d.inds[r] - 1; ci.ssgn[r] = 1.0; ci.soff[r] = d.params[r]; }
      break;
    case TO_CON_BOUND: {
      if (d.sense != TO_CONE_NEGATIVE_ORTHANT) return fail(TO_ERR_ARGUMENT, "BoundConstraint sense must be Inequality");
      if (d.n_params != 2 * nz) return dimerr("BoundConstraint needs z_max and z_min of length n+m");
      for (int i = 0; i < nz; ++i)
        if (!(d.params[i] >= d.params[nz + i])) return fail(TO_ERR_ARGUMENT, "Upper bounds must be greater than or equal to lower bounds");  // src/constraints.jl:712
      ci.width = nz; ci.selector = 1;
      for (int j = 0; j < nz; ++j) if (std::isfinite(d.params[j])) { if (p < TO_MAX_P) { ci.sidx[p] = j; ci.ssgn[p] = 1.0; ci.soff[p] = d.params[j]; } ++p; }
      for (int j = 0; j < nz; ++j) if (std::isfinite(d.params[nz + j])) { if (p < TO_MAX_P) { ci.sidx[p] = j; ci.ssgn[p] = -1.0; ci.soff[p] = d.params[nz + j]; } ++p; }
      break;
    }
    case TO_CON_NORM:
      if (d.n_params != 1) return fail(TO_ERR_ARGUMENT, "NormConstraint needs one parameter (val)");
      if (!(d.params[0] >= 0)) return fail(TO_ERR_ASSERTION, "Value must be greater than or equal to zero");  // src/constraints.jl:453
      if (d.sense != TO_CONE_ZERO && d.sense != TO_CONE_NEGATIVE_ORTHANT && d.sense != TO_CONE_SECOND_ORDER)
        return fail(TO_ERR_ARGUMENT, "NormConstraint sense must be Equality, Inequality or SecondOrderCone");
      if (d.n_inds < 1 || d.n_inds > nz) return dimerr("NormConstraint needs 1..n+m indices");
      for (int i = 0; i < d.n_inds; ++i) if (d.inds[i] < 1 || d.inds[i] > nz) return dimerr("NormConstraint index outside [x;u]");
      ci.width = nz;
      if (d.sense == TO_CONE_SECOND_ORDER) {
        p = d.n_inds + 1; ci.selector = 1;
        for (int r = 0; r < d.n_inds; ++r) { ci.sidx[r] = d.inds[r] - 1; ci.ssgn[r] = 1.0; ci.soff[r] = 0.0; }
        ci.sidx[d.n_inds] = -1; ci.ssgn[d.n_inds] = 0.0; ci.soff[d.n_inds] = d.params[0];
      } else p = 1;
      break;
    case TO_CON_CIRCLE:
      if (d.sense != TO_CONE_NEGATIVE_ORTHANT) return fail(TO_ERR_ARGUMENT, "CircleConstraint sense must be Inequality");
      if (d.n_inds != 2 || d.n_params % 3 != 0 || d.n_params == 0) return fail(TO_ERR_ASSERTION, "Lengths of xc, yc, and radius must be equal.");
      for (int i = 0; i < 2; ++i) if (d.inds[i] < 1 || d.inds[i] > n) return dimerr("CircleConstraint index outside the state");
      ci.width = n; p = d.n_params / 3;
      break;
    case TO_CON_SPHERE:
      if (d.sense != TO_CONE_NEGATIVE_ORTHANT) return fail(TO_ERR_ARGUMENT, "SphereConstraint sense must be Inequality");
      if (d.n_inds != 3 || d.n_params % 4 != 0 || d.n_params == 0) return fail(TO_ERR_ASSERTION, "Lengths of xc, yc, zc, and radius must be equal.");
      for (int i = 0; i < 3; ++i) if (d.inds[i] < 1 || d.inds[i] > n) return dimerr("SphereConstraint index outside the state");
      ci.width = n; p = d.n_params / 4;
      break;
    case TO_CON_LINEAR:
      if (d.sense != TO_CONE_ZERO && d.sense != TO_CONE_NEGATIVE_ORTHANT) return fail(TO_ERR_ARGUMENT, "LinearConstraint sense must be Equality or Inequality");
      if (d.n_inds < 1 || d.n_inds > nz || d.n_params == 0 || d.n_params % (d.n_inds + 1) != 0) return fail(TO_ERR_ASSERTION, "size(A,1) == length(b)");
      for (int i = 0; i < d.n_inds; ++i) if (d.inds[i] < 1 || d.inds[i] > nz) return dimerr("LinearConstraint index outside [x;u]");
      ci.width = nz; p = d.n_params / (d.n_inds + 1);
      break;
    case TO_CON_COLLISION:
      if (d.sense != TO_CONE_NEGATIVE_ORTHANT) return fail(TO_ERR_ARGUMENT, "CollisionConstraint sense must be Inequality");
      if (d.n_inds < 2 || d.n_inds % 2 != 0) return fail(TO_ERR_ASSERTION, "Position dimensions must be of equal length"); /* src/constraints.jl:349 */
      if (d.n_inds > n) return dimerr("CollisionConstraint has more position indices than states");
      if (d.n_params != 1) return fail(TO_ERR_ARGUMENT, "CollisionConstraint needs one parameter (radius)");
      for (int i = 0; i < d.n_inds; ++i) if (d.inds[i] < 1 || d.inds[i] > n) return fail(TO_ERR_DIMENSION_MISMATCH, "CollisionConstraint index outside state");
      ci.width = n; p = 1; break;
    case TO_CON_QUATVEC:
      if (d.sense != TO_CONE_ZERO) return fail(TO_ERR_ARGUMENT, "QuatVecEq sense must be Equality");
      if (d.n_inds != 4 || d.n_params != 4) return fail(TO_ERR_ARGUMENT, "QuatVecEq needs 4 quaternion indices and a 4-vector qf");
      for (int i = 0; i < 4; ++i) if (d.inds[i] < 1 || d.inds[i] > n) return fail(TO_ERR_DIMENSION_MISMATCH, "QuatVecEq index outside state");
      ci.width = n; p = 3; break;
    default: return fail(TO_ERR_UNSUPPORTED, "unknown constraint kind");
  }
  if (p < 1 || p > TO_MAX_P) return fail(TO_ERR_UNSUPPORTED, "constraint output dimension outside 1..TO_MAX_P");
  if (ci.selector && (d.kind == TO_CON_GOAL || (d.kind == TO_CON_NORM && d.sense == TO_CONE_SECOND_ORDER))) {
    // fast layouts: rows map to a state prefix z[r] or to the control block z[n+r] with sign +1 (see problem_dev.h)
    const int D = d.n_inds;
    bool prefix = D <= n, ctrl = D <= m;
    for (int r = 0; r < D; ++r) { prefix = prefix && d.inds[r] == r + 1; ctrl = ctrl && d.inds[r] == n + r + 1; }
    ci.fast = prefix ? 1 : ctrl ? 2 : 0;
  }
  if (d.p != 0 && d.p != p) return fail(TO_ERR_DIMENSION_MISMATCH, "constraint output dimension does not match its descriptor");
  ci.p = p; ci.k1 = d.k_first - 1; ci.k2 = d.k_last - 1;
  *out = ci;
  return TO_OK;
}

// THE host image of the per-trajectory tables that carry a spare tile (DevProblem::pm, dtb, cl, gw, ga; handle.h names the other family).
// values[L, B], row fastest, one column per trajectory -> entry e of trajectory b at tiled[((b >> 6) * L + e) * 64 + (b & 63)], the address every
// kernel forms: Bp / 64 tiles and one spare tile (like the nominal states).  Every lane behind the batch, and the whole spare tile, holds the
// SHARED value of its row, shared[L] (idle lanes compute along on valid data).  values == NULL: the shared row for every trajectory.
inline size_t tiled_len(size_t L, int Bp) { return ((size_t)Bp / 64 + 1) * L * 64; }
inline void tile_rows(size_t L, int B, int Bp, const double* values, const double* shared, std::vector<double>* tiled) {
  const size_t tiles = (size_t)Bp / 64 + 1;
  tiled->resize(tiled_len(L, Bp));
  for (size_t t = 0; t < tiles; ++t)
    for (size_t e = 0; e < L; ++e)
      for (int l = 0; l < 64; ++l) {
        const size_t b = t * 64 + l;
        (*tiled)[(t * L + e) * 64 + l] = (values && b < (size_t)B) ? values[L * b + e] : shared[e];
      }
}

// Per-trajectory limits of a selector constraint (to_set_constraint_limits_batch).  constraint_limits_q: the number of values per
// trajectory — p for a BoundConstraint (one per finite row, in row order), 1 for a second-order-cone NormConstraint (the value of its last
// row) — or the refusal for every other kind.  lower_constraint_limits: limits[q, B] -> the values of soff[r] for every row, rows[p, B]
// (what DevProblem::cl holds), with the checks the reference's constructors make on a single constraint, for every trajectory.
inline int constraint_limits_q(const DevCon& ci, int* q) {
  if (ci.d.kind == TO_CON_BOUND) { *q = ci.p; return TO_OK; }
  if (ci.d.kind == TO_CON_NORM && ci.d.sense == TO_CONE_SECOND_ORDER) { *q = 1; return TO_OK; }
  return fail(TO_ERR_UNSUPPORTED, "per-trajectory constraint limits: BoundConstraint (its bounds) and NormConstraint with SecondOrderCone (its value) only");
}
inline int lower_constraint_limits(const DevCon& ci, int B, const double* limits, std::vector<double>* rows) {
  int q = 0;
  if (int r = constraint_limits_q(ci, &q)) return r;
  const int p = ci.p;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < q; ++i)
      if (!std::isfinite(limits[i + (size_t)q * b]))
        return fail(TO_ERR_ARGUMENT, "to_set_constraint_limits_batch: value " + std::to_string(i) + " of trajectory " + std::to_string(b) + " is not finite");
  rows->assign((size_t)p * B, 0.0);
  if (ci.d.kind == TO_CON_BOUND) {
    for (int b = 0; b < B; ++b) {
      const double* lb = limits + (size_t)p * b;
      for (int r = 0; r < p; ++r) {
        if (ci.ssgn[r] > 0.0)  // an upper row: against the lower row of the same coordinate, if there is one
          for (int s = 0; s < p; ++s)
            if (ci.ssgn[s] < 0.0 && ci.sidx[s] == ci.sidx[r] && !(lb[r] >= lb[s]))
              return fail(TO_ERR_ARGUMENT, "Upper bounds must be greater than or equal to lower bounds (trajectory " + std::to_string(b) + ")");  // src/constraints.jl:712
        (*rows)[r + (size_t)p * b] = lb[r];
      }
    }
  } else {
    for (int b = 0; b < B; ++b) {
      if (!(limits[b] >= 0)) return fail(TO_ERR_ASSERTION, "Value must be greater than or equal to zero (trajectory " + std::to_string(b) + ")");  // src/constraints.jl:451
      (*rows)[(p - 1) + (size_t)p * b] = limits[b];  // (rows r < p - 1 select a coordinate: offset 0)
    }
  }
  return TO_OK;
}
// the descriptor's own limits in the layout of the setter's argument (what the getter reports for a constraint on shared limits)
inline void shared_constraint_limits(const DevCon& ci, int q, double* out) {
  for (int i = 0; i < q; ++i) out[i] = ci.soff[q == 1 && ci.d.kind == TO_CON_NORM ? ci.p - 1 : i];
}
// The table behind DevProblem::cl holds the rows of EVERY constraint, L = n_cl = their summed p.  constraint_limits_bases: the first row of every
// constraint's block (returns n_cl); constraint_limits_shared: the shared row, every constraint's soff[0 .. p) at its base; constraint_limits_values:
// values[n_cl, B] for tile_rows — the block of a constraint that was given limits (given[i], [q, B], not empty) through lower_constraint_limits,
// the block of every other one on its soff.
inline int constraint_limits_bases(const std::vector<DevCon>& cons, std::vector<int>* base) {
  base->assign(cons.size(), 0);
  int L = 0;
  for (size_t i = 0; i < cons.size(); ++i) { (*base)[i] = L; L += cons[i].p; }
  return L;
}
inline void constraint_limits_shared(const std::vector<DevCon>& cons, const std::vector<int>& base, int n_cl, std::vector<double>* shared) {
  shared->assign((size_t)n_cl, 0.0);
  for (size_t i = 0; i < cons.size(); ++i)
    for (int r = 0; r < cons[i].p; ++r) (*shared)[base[i] + r] = cons[i].soff[r];
}
inline int constraint_limits_values(const std::vector<DevCon>& cons, const std::vector<std::vector<double>>& given, const std::vector<int>& base,
                                    const std::vector<double>& shared, int B, std::vector<double>* values) {
  const size_t n_cl = shared.size();
  values->resize(n_cl * B);
  for (int b = 0; b < B; ++b) std::copy(shared.begin(), shared.end(), values->begin() + n_cl * b);
  std::vector<double> rows;
  for (size_t i = 0; i < cons.size(); ++i) {
    if (given[i].empty()) continue;
    const int p = cons[i].p;
    if (int r = lower_constraint_limits(cons[i], B, given[i].data(), &rows)) return r;
    for (int b = 0; b < B; ++b) std::copy(rows.begin() + (size_t)p * b, rows.begin() + (size_t)p * (b + 1), values->begin() + n_cl * b + base[i]);
  }
  return TO_OK;
}

// One tracking reference per trajectory (to_set_tracking_reference_batch / to_set_tracking_window): every refusal of the two entry points,
// decided from what the host knows of the handle before any device call.  TrackFacts: those facts (model_key as in handle.h ModelOps: 7 the
// hybrid double integrator, 8 model vectors, 9 .. 11 InfeasibleModel; Nref_set = 0 while no reference is stored).
struct TrackFacts {
  int model_key; const char* model_name;
  int n, m, N, B;
  const to_cost_desc* costs; int n_costs; const int* cost_index /* [N] */;
  bool in_flight;
  int Nref_set, end_mode_set;
  bool cost_weights = false;  // the CALLER set weights (to_set_cost_weights_batch; CostLaneState::weights): k_track_lower forms -Q x_ref from the DESCRIPTOR's Q
};
// the window itself: start[B] (NULL: 1 for all) against a reference of Nref knots
inline int validate_tracking_starts(const char* who, int N, int B, int Nref, int end_mode, const int32_t* start) {
  for (int b = 0; b < B; ++b) {
    const long long s = start ? start[b] : 1;
    if (s < 1) return fail(TO_ERR_ARGUMENT, std::string(who) + ": start of trajectory " + std::to_string(b) + " is " + std::to_string(s) + " (1-based: must be >= 1)");
    if (end_mode == TO_TRACK_END_HOLD && s > Nref)
      return fail(TO_ERR_ARGUMENT, std::string(who) + ": start of trajectory " + std::to_string(b) + " is " + std::to_string(s) + ", behind the reference (Nref = " +
                                       std::to_string(Nref) + ")");
    if (end_mode == TO_TRACK_END_REFUSE && s - 1 + N > Nref)  // update_trajectory!'s BoundsError (src/objective.jl:198-212)
      return fail(TO_ERR_ARGUMENT, std::string(who) + ": reference trajectory too short for trajectory " + std::to_string(b) + ": start " + std::to_string(s) +
                                       " - 1 + N = " + std::to_string(s - 1 + N) + " > Nref = " + std::to_string(Nref) + " (TO_TRACK_END_HOLD tracks the last knot instead)");
  }
  return TO_OK;
}
// what both entry points ask of the handle: idle, a model whose knots share one state, a cost of its own on every knot, no ErrorQuadratic
inline int validate_tracking_target(const char* who, const TrackFacts& f) {
  if (f.in_flight) return fail(TO_ERR_ARGUMENT, "an asynchronous solve is in flight on this handle (call to_solve_wait first)");
  if (f.model_key >= 7)
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": not available for the " + f.model_name +
                                        " (TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, TO_MODEL_VECTOR and TO_MODEL_INFEASIBLE have no per-trajectory tracking reference)");
  if (f.cost_weights)
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": the handle carries per-trajectory cost weights (to_set_cost_weights_batch); the reference is lowered "
                                        "with the descriptors' Q and R (to_clear_cost_weights_batch first)");
  for (int k = 0; k < f.N; ++k)
    for (int l = k + 1; l < f.N; ++l)
      if (f.cost_index[k] == f.cost_index[l])
        return fail(TO_ERR_ARGUMENT, std::string(who) + " needs a tracking objective (a distinct cost per knot): knots " + std::to_string(k + 1) + " and " +
                                         std::to_string(l + 1) + " share cost " + std::to_string(f.cost_index[k]));
  for (int k = 0; k < f.N; ++k)
    if (f.costs[f.cost_index[k]].kind == TO_COST_ERROR_QUADRATIC)
      return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": the cost of knot " + std::to_string(k + 1) + " is ErrorQuadratic (its q slot carries x_ref)");
  return TO_OK;
}
inline int validate_tracking_reference(const TrackFacts& f, int Nref, const double* Xref, const double* Uref, const int32_t* start, int end_mode) {
  const char* who = "to_set_tracking_reference_batch";
  if (f.in_flight) return validate_tracking_target(who, f);
  if (!Xref) return fail(TO_ERR_NULL, std::string(who) + ": Xref is NULL");
  if (int r = validate_tracking_target(who, f)) return r;
  if (Nref < 1) return fail(TO_ERR_ARGUMENT, std::string(who) + ": Nref must be >= 1; got " + std::to_string(Nref));
  if (end_mode != TO_TRACK_END_REFUSE && end_mode != TO_TRACK_END_HOLD)
    return fail(TO_ERR_ARGUMENT, std::string(who) + ": end_mode must be TO_TRACK_END_REFUSE (0) or TO_TRACK_END_HOLD (1)");
  for (int b = 0; b < f.B; ++b)
    for (int j = 0; j < Nref; ++j) {
      bool ok = true;
      for (int i = 0; i < f.n; ++i) ok = ok && std::isfinite(Xref[i + (size_t)f.n * (j + (size_t)Nref * b)]);
      for (int i = 0; Uref && i < f.m; ++i) ok = ok && std::isfinite(Uref[i + (size_t)f.m * (j + (size_t)Nref * b)]);
      if (!ok) return fail(TO_ERR_ARGUMENT, std::string(who) + ": the reference of trajectory " + std::to_string(b) + " is not finite at knot " + std::to_string(j + 1));
    }
  return validate_tracking_starts(who, f.N, f.B, Nref, end_mode, start);
}
inline int validate_tracking_window(const TrackFacts& f, const int32_t* start) {
  const char* who = "to_set_tracking_window";
  if (f.in_flight) return validate_tracking_target(who, f);
  if (!start) return fail(TO_ERR_NULL, std::string(who) + ": start is NULL");
  if (f.Nref_set < 1) return fail(TO_ERR_ARGUMENT, std::string(who) + ": no tracking reference is set (to_set_tracking_reference_batch first)");
  if (int r = validate_tracking_target(who, f)) return r;
  return validate_tracking_starts(who, f.N, f.B, f.Nref_set, f.end_mode_set, start);
}
// the reference in the layout upload_vec takes: rows [x_ref[j]; u_ref[j]] (u rows zero without Uref), [(n+m) Nref, B]
inline void pack_tracking_reference(int n, int m, int B, int Nref, const double* Xref, const double* Uref, std::vector<double>* out) {
  const int nz = n + m;
  out->assign((size_t)nz * Nref * B, 0.0);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < Nref; ++j) {
      double* z = out->data() + (size_t)nz * (j + (size_t)Nref * b);
      for (int i = 0; i < n; ++i) z[i] = Xref[i + (size_t)n * (j + (size_t)Nref * b)];
      for (int i = 0; Uref && i < m; ++i) z[n + i] = Uref[i + (size_t)m * (j + (size_t)Nref * b)];
    }
}

// The dual shift of the receding-horizon loop (to_mpc_shift_duals): every refusal of the entry point, decided from what the host knows of the
// handle before any device call (model_key as in TrackFacts).  A handle without constraints passes: the entry point then launches nothing.
struct MpcDualFacts {
  int model_key; const char* model_name;
  int N, B;
  bool in_flight;
};
inline int validate_mpc_shift_duals(const MpcDualFacts& f, int32_t shift, int32_t tail, const int32_t* action /* [B] or NULL */) {
  const char* who = "to_mpc_shift_duals";
  if (f.in_flight) return fail(TO_ERR_ARGUMENT, "an asynchronous solve is in flight on this handle (call to_solve_wait first)");
  if (f.model_key >= 7)  // the models to_mpc_advance refuses: their plan cannot move, so neither can its multipliers
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": not available for the " + f.model_name +
                                        " (TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, TO_MODEL_VECTOR and TO_MODEL_INFEASIBLE cannot shift their plan)");
  if (shift < 1 || shift > f.N - 2)
    return fail(TO_ERR_ARGUMENT, std::string(who) + ": shift must be in 1 .. N-2 = " + std::to_string(f.N - 2) + "; got " + std::to_string(shift));
  if (tail != TO_MPC_DUAL_TAIL_HOLD && tail != TO_MPC_DUAL_TAIL_ZERO)
    return fail(TO_ERR_ARGUMENT, std::string(who) + ": tail must be TO_MPC_DUAL_TAIL_HOLD (0) or TO_MPC_DUAL_TAIL_ZERO (1)");
  for (int b = 0; action && b < f.B; ++b)
    if (action[b] != TO_MPC_DUAL_LEAVE && action[b] != TO_MPC_DUAL_SHIFT && action[b] != TO_MPC_DUAL_RESET)
      return fail(TO_ERR_ARGUMENT, std::string(who) + ": action of trajectory " + std::to_string(b) + " is " + std::to_string(action[b]) +
                                       " (TO_MPC_DUAL_LEAVE 0, TO_MPC_DUAL_SHIFT 1 or TO_MPC_DUAL_RESET 2)");
  return TO_OK;
}

// Per-trajectory time steps (to_set_time_steps_batch): dt[(N-1), B], knot fastest, column b read exactly like to_problem_desc::dt.
// validate_time_steps checks every value — finite and > 0, the check the descriptor's own steps get at to_create; there is NO "must sum to
// tf - t0" check: trajectory b ends at its own tf_b = t0 + sum_k dt_b[k].  lower_time_steps: the checks, then the image of DevProblem::dtb
// (tile_rows with L = N - 1; the shared row: the descriptor's steps); a refused call leaves the output untouched.
inline int validate_time_steps(int N, int B, const double* dt) {
  const int L = N - 1;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < L; ++k) {
      const double v = dt[k + (size_t)L * b];
      if (!std::isfinite(v) || !(v > 0.0))
        return fail(TO_ERR_ARGUMENT, "to_set_time_steps_batch: time step " + std::to_string(k) + " of trajectory " + std::to_string(b) +
                                         (std::isfinite(v) ? " is not > 0" : " is not finite"));
    }
  return TO_OK;
}
inline size_t time_steps_tiled_len(int N, int Bp) { return tiled_len((size_t)N - 1, Bp); }
inline int lower_time_steps(int N, int B, int Bp, const double* dt, const double* shared /* [N-1] */, std::vector<double>* tiled) {
  if (int r = validate_time_steps(N, B, dt)) return r;
  tile_rows((size_t)N - 1, B, Bp, dt, shared, tiled);
  return TO_OK;
}

// Per-trajectory cost weights (to_set_cost_weights_batch / to_get_... / to_clear_...): every refusal of the three entry points, decided from what
// the host knows of the handle before any device call.  CostWeightFacts: those facts (model_key as in TrackFacts; NULL facts: a NULL handle).
// The VALUES are held to what to_set_cost asks of a descriptor's Q and R and to being finite, nothing more: the reference only warns about
// definiteness (src/cost_functions.jl:337-343), and a weight of zero or below is the caller's business here as it is in a descriptor.
struct CostWeightFacts {
  int model_key; const char* model_name;
  int n, m, B;
  const to_cost_desc* costs; int n_costs;
  bool in_flight;
  int Nref_set;  // knots of a stored tracking reference (0: none)
};
inline const char* cost_kind_name(int kind) {
  return kind == TO_COST_DIAGONAL ? "DiagonalCost" : kind == TO_COST_QUADRATIC ? "QuadraticCost" : kind == TO_COST_DIAGONAL_QUAT ? "DiagonalQuatCost"
         : kind == TO_COST_ERROR_QUADRATIC ? "ErrorQuadratic" : "unknown cost kind";
}
// the handle as a target (all three entry points; cost_id < 0 with any = true: the clear call, which names no cost)
inline int validate_cost_weights_target(const char* who, const CostWeightFacts* f, int32_t cost_id, bool any = false) {
  if (!f) return fail(TO_ERR_NULL, "null handle");
  if (f->in_flight) return fail(TO_ERR_ARGUMENT, "an asynchronous solve is in flight on this handle (call to_solve_wait first)");
  if (f->model_key >= 7)
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": per-trajectory cost weights are not available for the " + f->model_name +
                                        " (TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, TO_MODEL_VECTOR and TO_MODEL_INFEASIBLE share their weights)");
  if (any) return TO_OK;
  if (cost_id < 0 || cost_id >= f->n_costs) return fail(TO_ERR_ARGUMENT, "cost id out of range");
  return TO_OK;
}
inline int validate_cost_weights_kind(const char* who, const CostWeightFacts& f, int32_t cost_id) {
  const int kind = f.costs[cost_id].kind;
  if (kind != TO_COST_DIAGONAL && kind != TO_COST_DIAGONAL_QUAT)
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": cost " + std::to_string(cost_id) + " is of kind " + cost_kind_name(kind) +
                                        "; per-trajectory weights are the diagonal Q and R of DiagonalCost and DiagonalQuatCost only");
  return TO_OK;
}
inline int validate_cost_weights(const CostWeightFacts* f, int32_t cost_id, const double* Q /* [n, B] or NULL */, const double* R /* [m, B] or NULL */) {
  const char* who = "to_set_cost_weights_batch";
  if (int r = validate_cost_weights_target(who, f, cost_id)) return r;
  if (!Q && !R) return fail(TO_ERR_ARGUMENT, std::string(who) + ": Q and R are both NULL");
  if (int r = validate_cost_weights_kind(who, *f, cost_id)) return r;
  if (f->Nref_set > 0)
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": the handle holds a tracking reference (to_set_tracking_reference_batch), which is lowered with the "
                                        "descriptors' Q and R (to_clear_tracking_reference_batch first)");
  for (int b = 0; b < f->B; ++b) {
    for (int i = 0; Q && i < f->n; ++i)
      if (!std::isfinite(Q[i + (size_t)f->n * b]))
        return fail(TO_ERR_ARGUMENT, std::string(who) + ": Q[" + std::to_string(i) + "] of trajectory " + std::to_string(b) + " is not finite");
    for (int j = 0; R && j < f->m; ++j)
      if (!std::isfinite(R[j + (size_t)f->m * b]))
        return fail(TO_ERR_ARGUMENT, std::string(who) + ": R[" + std::to_string(j) + "] of trajectory " + std::to_string(b) + " is not finite");
  }
  return TO_OK;
}
inline int validate_cost_weights_get(const CostWeightFacts* f, int32_t cost_id, const double* Q, const double* R) {
  const char* who = "to_get_cost_weights_batch";
  if (int r = validate_cost_weights_target(who, f, cost_id)) return r;
  if (!Q && !R) return fail(TO_ERR_ARGUMENT, std::string(who) + ": Q and R are both NULL");
  return validate_cost_weights_kind(who, *f, cost_id);
}
// The host copy behind DevProblem::gw: values[L, B] with L = n_costs (n + m), row ci (n + m) + i of column b = Q_i (i < n) / R_{i-n} of cost ci
// as trajectory b is evaluated with it.  cost_weights_fill: every cost's descriptor values (first use; cost_weights_restart: one cost's rows
// again, behind to_set_cost); cost_weights_store: the setter's Q / R into one cost's rows; cost_weights_shared: the shared row of the device
// image (tile_rows) — the descriptors' diagonals, one column of what cost_weights_fill writes.  A dense cost's rows are never read; they hold the
// leading entries of its arrays.
inline void cost_weights_restart(int n, int m, int B, const to_cost_desc* costs, int n_costs, int ci, std::vector<double>* values) {
  const int nz = n + m;
  const size_t L = (size_t)n_costs * nz;
  for (int b = 0; b < B; ++b) {
    double* v = values->data() + L * b + (size_t)ci * nz;
    for (int i = 0; i < n; ++i) v[i] = costs[ci].Q[i];
    for (int j = 0; j < m; ++j) v[n + j] = costs[ci].R[j];
  }
}
inline void cost_weights_fill(int n, int m, int B, const to_cost_desc* costs, int n_costs, std::vector<double>* values) {
  values->assign((size_t)n_costs * (n + m) * B, 0.0);
  for (int ci = 0; ci < n_costs; ++ci) cost_weights_restart(n, m, B, costs, n_costs, ci, values);
}
inline void cost_weights_store(int n, int m, int B, int n_costs, int ci, const double* Q, const double* R, std::vector<double>* values) {
  const int nz = n + m;
  const size_t L = (size_t)n_costs * nz;
  for (int b = 0; b < B; ++b) {
    double* v = values->data() + L * b + (size_t)ci * nz;
    for (int i = 0; Q && i < n; ++i) v[i] = Q[i + (size_t)n * b];
    for (int j = 0; R && j < m; ++j) v[n + j] = R[j + (size_t)m * b];
  }
}
inline void cost_weights_shared(int n, int m, const to_cost_desc* costs, int n_costs, std::vector<double>* shared) {
  cost_weights_fill(n, m, 1, costs, n_costs, shared);
}
// the image as one call (what tests/host_shim/cost_weights_harness.cpp checks lane by lane): the shared row, then tile_rows
inline size_t cost_weights_tiled_len(int n, int m, int n_costs, int Bp) { return tiled_len((size_t)n_costs * (n + m), Bp); }
inline void cost_weights_tile(int n, int m, int B, int Bp, const to_cost_desc* costs, int n_costs, const std::vector<double>& values, std::vector<double>* tiled) {
  std::vector<double> shared;
  cost_weights_shared(n, m, costs, n_costs, &shared);
  tile_rows(shared.size(), B, Bp, values.data(), shared.data(), tiled);
}

// Per-trajectory attitude references (to_set_cost_attitude_batch / to_get_... / to_clear_..., to_set_tracking_attitude): every refusal, decided from
// what the host knows of the handle before any device call, the image of DevProblem::ga, and the rules by which ga rides on gw.  The facts are
// CostWeightFacts (the target rules are those of the weights: the same models are refused).  The VALUES are used as given — QuatLQRCost does
// not normalise xf[quat_ind] either (src/lie_costs.jl:134-141), and the sign is immaterial under min(1 +- dq) — and only held to being finite.
inline int validate_cost_attitude_kind(const char* who, const CostWeightFacts& f, int32_t cost_id) {
  const int kind = f.costs[cost_id].kind;
  if (kind != TO_COST_DIAGONAL_QUAT)
    return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": cost " + std::to_string(cost_id) + " is of kind " + cost_kind_name(kind) +
                                        "; a per-trajectory attitude reference is the q_ref of a DiagonalQuatCost only" +
                                        (kind == TO_COST_ERROR_QUADRATIC ? " (an ErrorQuadratic keeps its reference in its q slot)" : ""));
  return TO_OK;
}
inline int validate_cost_attitude(const CostWeightFacts* f, int32_t cost_id, const double* q_ref /* [4, B] */) {
  const char* who = "to_set_cost_attitude_batch";
  if (!f) return fail(TO_ERR_NULL, "null handle");
  if (!q_ref) return fail(TO_ERR_NULL, std::string(who) + ": q_ref is NULL");
  if (int r = validate_cost_weights_target(who, f, cost_id)) return r;
  if (int r = validate_cost_attitude_kind(who, *f, cost_id)) return r;
  for (int b = 0; b < f->B; ++b)
    for (int i = 0; i < 4; ++i)
      if (!std::isfinite(q_ref[i + (size_t)4 * b]))
        return fail(TO_ERR_ARGUMENT, std::string(who) + ": q_ref[" + std::to_string(i) + "] of trajectory " + std::to_string(b) + " is not finite");
  return TO_OK;
}
inline int validate_cost_attitude_get(const CostWeightFacts* f, int32_t cost_id, const double* q_ref) {
  const char* who = "to_get_cost_attitude_batch";
  if (!f) return fail(TO_ERR_NULL, "null handle");
  if (!q_ref) return fail(TO_ERR_NULL, std::string(who) + ": q_ref is NULL");
  if (int r = validate_cost_weights_target(who, f, cost_id)) return r;
  return validate_cost_attitude_kind(who, *f, cost_id);
}
// to_set_tracking_attitude: on needs a stored reference and a DiagonalQuatCost among the tracked costs (those of cost_index[0 .. N-1])
inline int validate_tracking_attitude(const TrackFacts* f, int32_t on) {
  const char* who = "to_set_tracking_attitude";
  if (!f) return fail(TO_ERR_NULL, "null handle");
  if (f->in_flight) return fail(TO_ERR_ARGUMENT, "an asynchronous solve is in flight on this handle (call to_solve_wait first)");
  if (on != 0 && on != 1) return fail(TO_ERR_ARGUMENT, std::string(who) + ": on must be 0 or 1; got " + std::to_string(on));
  if (!on) return TO_OK;
  if (f->Nref_set < 1) return fail(TO_ERR_ARGUMENT, std::string(who) + ": no tracking reference is set (to_set_tracking_reference_batch first)");
  for (int k = 0; k < f->N; ++k)
    if (f->costs[f->cost_index[k]].kind == TO_COST_DIAGONAL_QUAT) return TO_OK;
  return fail(TO_ERR_UNSUPPORTED, std::string(who) + ": none of the tracked costs is a DiagonalQuatCost (a reference attitude is the q_ref of that kind only)");
}
// The image of DevProblem::ga: L = 4 n_costs rows per trajectory, row 4 ci + i = q_ref[i] of cost ci (a cost of another kind carries its
// descriptor's q_ref slot, which is never read).  cost_attitude_fill: every cost's descriptor values as a host array [L, B] (first use);
// cost_attitude_rows: one cost's rows alone, [4, B] (to_set_cost, the clears); cost_attitude_shared: the shared row of the device image
// (tile_rows), one column of what cost_attitude_fill writes — the library's uploads are that row for every trajectory.  After the first upload the
// DEVICE array is the truth (k_track_lower writes it): the setter, the getter and the restarts move one cost's four rows and nothing else.
inline void cost_attitude_rows(int B, const to_cost_desc& c, std::vector<double>* rows) {
  rows->resize((size_t)4 * B);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 4; ++i) (*rows)[i + (size_t)4 * b] = c.q_ref[i];
}
inline void cost_attitude_fill(int B, const to_cost_desc* costs, int n_costs, std::vector<double>* values) {
  const size_t L = (size_t)4 * n_costs;
  values->assign(L * B, 0.0);
  for (int b = 0; b < B; ++b)
    for (int ci = 0; ci < n_costs; ++ci)
      for (int i = 0; i < 4; ++i) (*values)[L * b + 4 * ci + i] = costs[ci].q_ref[i];
}
inline void cost_attitude_shared(const to_cost_desc* costs, int n_costs, std::vector<double>* shared) { cost_attitude_fill(1, costs, n_costs, shared); }
// the image as one call (tests/host_shim/attitude_harness.cpp): the shared row, then tile_rows
inline size_t cost_attitude_tiled_len(int n_costs, int Bp) { return tiled_len((size_t)4 * n_costs, Bp); }
inline void cost_attitude_tile(int B, int Bp, const to_cost_desc* costs, int n_costs, const std::vector<double>& values, std::vector<double>* tiled) {
  std::vector<double> shared;
  cost_attitude_shared(costs, n_costs, &shared);
  tile_rows(shared.size(), B, Bp, values.data(), shared.data(), tiled);
}
// (How ga rides on gw — which of the two arrays a call fills, when both are released — is path_plan.h cost_lane_step.)

// rot: attitude representation of the model's state (to_rotation), -1 for vector-space models
inline int validate_cost(int n, int rot, const to_cost_desc& c) {
  if (c.kind != TO_COST_DIAGONAL && c.kind != TO_COST_QUADRATIC && c.kind != TO_COST_DIAGONAL_QUAT && c.kind != TO_COST_ERROR_QUADRATIC)
    return fail(TO_ERR_UNSUPPORTED, "unknown cost kind");
  if (c.kind == TO_COST_ERROR_QUADRATIC) {  // needs the rigid-body state layout [r; attitude; v; w]
    if (rot < 0) return fail(TO_ERR_ARGUMENT, "ErrorQuadratic needs a rigid-body model");
    if ((int)c.w != rot || c.w != (double)rot) return fail(TO_ERR_ARGUMENT, "ErrorQuadratic: w must name the model's attitude representation (to_rotation)");
    if (rot == TO_ROT_QUATERNION)
      for (int i = 0; i < 4; ++i) if (c.q_ind[i] != 4 + i) return fail(TO_ERR_UNSUPPORTED, "ErrorQuadratic: q_ind must be 4:7");
  }
  if (c.kind == TO_COST_DIAGONAL_QUAT) {
    if (rot > TO_ROT_QUATERNION) return fail(TO_ERR_ARGUMENT, "DiagonalQuatCost needs a state that carries a unit quaternion");
    for (int i = 0; i < 4; ++i) if (c.q_ind[i] < 1 || c.q_ind[i] > n) return fail(TO_ERR_DIMENSION_MISMATCH, "quat_ind outside the state");
  }
  return TO_OK;
}

// The whole problem descriptor (to_create): every check and every host table, before the entry point asks for a device.  A refused call leaves
// *out untouched (as with every routine below).
struct LoweredProblem {
  int n = 0, m = 0, ne = 0, key = -1;
  std::vector<double> dt, step_table;  // [N-1]; TO_MODEL_VECTOR: the per-step model table (models.h ModelVectorModel), else empty
  std::vector<int> cost_index;         // [N]
  std::vector<DevCon> cons;
  long long n_duals = 0;
};
inline int lower_problem(const to_problem_desc* desc, const to_solver_opts* opts /* may be NULL */, LoweredProblem* out) {
  if (!desc) return fail(TO_ERR_NULL, "null descriptor");
  if (desc->abi_version != TO_ABI_VERSION) return fail(TO_ERR_ARGUMENT, "ABI version mismatch");
  if (opts) if (int r = validate_opts(*opts)) return r;
  LoweredProblem lp;
  int& n = lp.n; int& m = lp.m;
  if (model_dims(desc->model, desc->model_params, &n, &m, &lp.ne, &lp.key)) return fail(TO_ERR_UNSUPPORTED, "unknown model");
  if (desc->n != n || desc->m != m) return fail(TO_ERR_DIMENSION_MISMATCH, "Objective state/control dimensions don't match model.");  // src/problem.jl:65-68
  if (desc->N < 2) return fail(TO_ERR_ASSERTION, "length(models) == N-1 requires N >= 2");                                         // src/problem.jl:49
  if (desc->B < 1) return fail(TO_ERR_ARGUMENT, "batch must be positive");
  if (!(desc->tf > desc->t0)) return fail(TO_ERR_ASSERTION, "tf > t0");                                                             // src/problem.jl:50
  if (desc->integrator < TO_RK4 || desc->integrator > TO_EULER) return fail(TO_ERR_UNSUPPORTED, "unknown integrator");
  const int N = desc->N;
  std::vector<double>& dt = lp.dt;
  dt.resize(N - 1);
  if (desc->dt) {
    double s = 0;
    for (int k = 0; k < N - 1; ++k) { dt[k] = desc->dt[k]; s += dt[k]; if (!(dt[k] > 0)) return fail(TO_ERR_ASSERTION, "dt must be positive"); }
    if (std::fabs(s - (desc->tf - desc->t0)) > 1e-8 * std::fmax(1.0, std::fabs(desc->tf - desc->t0)))
      return fail(TO_ERR_ASSERTION, "time(Z[end]) ≈ tf: time steps are inconsistent with the final time");                          // src/problem.jl:52
  } else {
    for (int k = 0; k < N - 1; ++k) dt[k] = (desc->tf - desc->t0) / (N - 1);
  }
  if (desc->n_costs < 1 || !desc->costs) return fail(TO_ERR_ARGUMENT, "objective needs at least one cost function");
  const int rot = desc->model == TO_MODEL_QUADROTOR ? (int)desc->model_params[10] : -1;
  for (int i = 0; i < desc->n_costs; ++i) if (int r = validate_cost(n, rot, desc->costs[i])) return r;
  if (desc->model == TO_MODEL_HYBRID_DOUBLE_INTEGRATOR) {
    const double S = desc->model_params[1];
    if (!(S >= 1.0) || !(S <= (double)(N - 2)) || S != std::floor(S))
      return fail(TO_ERR_ARGUMENT, "hybrid double integrator: params[1] (time steps of the first model) must be an integer in 1 .. N-2");
  }
  if (desc->model == TO_MODEL_VECTOR) if (int r = lower_step_models(desc->step_models, N, &lp.step_table)) return r;  // validated like RD.dims(models)
  std::vector<int>& cost_index = lp.cost_index;
  cost_index.resize(N);
  if (desc->cost_index) {
    for (int k = 0; k < N; ++k) {
      if (desc->cost_index[k] < 0 || desc->cost_index[k] >= desc->n_costs) return fail(TO_ERR_DIMENSION_MISMATCH, "cost_index outside the cost list");
      cost_index[k] = desc->cost_index[k];
    }
  } else {
    if (desc->n_costs < 2) return fail(TO_ERR_ARGUMENT, "Objective(stage, terminal, N) needs two cost functions");
    for (int k = 0; k < N; ++k) cost_index[k] = (k == N - 1) ? 1 : 0;
  }
  if (desc->n_constraints < 0 || (desc->n_constraints > 0 && !desc->constraints)) return fail(TO_ERR_ARGUMENT, "bad constraint list");
  for (int i = 0; i < desc->n_constraints; ++i) {
    DevCon ci;
    if (int r = validate_constraint(n, m, N, desc->constraints[i], &ci)) return r;
    ci.dual_off = lp.n_duals;
    lp.n_duals += (long long)ci.p * (ci.k2 - ci.k1 + 1);
    lp.cons.push_back(ci);
  }
  *out = std::move(lp);
  return TO_OK;
}

// to_set_constraint_params_batch: params[p, B] -> the shift of z = [x; u] the constraint sees, shift[nz, B] (DevProblem::cp).  GOAL, params =
// xf_b[inds]: target xf + d is the shared constraint at x - d.  LINEAR, params = b_b: A z[inds] - (b + db) = A (z[inds] - dz) - b with the
// minimum-norm dz = A'(A A')^-1 db, which needs linearly independent rows.
inline int lower_constraint_params(const DevCon& ci, int nz, int B, const double* params /* [p, B] */, std::vector<double>* shift_out /* [nz, B] */) {
  if (ci.d.kind != TO_CON_GOAL && ci.d.kind != TO_CON_LINEAR)
    return fail(TO_ERR_UNSUPPORTED, "per-trajectory constraint parameters: GoalConstraint (its target) and LinearConstraint (its b) only");
  const int p = ci.p;
  std::vector<double> shift((size_t)nz * B, 0.0);
  if (ci.d.kind == TO_CON_GOAL) {
    for (int b = 0; b < B; ++b)
      for (int r = 0; r < p; ++r) shift[(size_t)(ci.d.inds[r] - 1) + (size_t)nz * b] = params[r + (size_t)p * b] - ci.d.params[r];
  } else {
    const int D = ci.d.n_inds;
    const double* A = ci.d.params;          // p x D, column-major
    const double* b0 = ci.d.params + (size_t)p * D;
    std::vector<double> G((size_t)p * p, 0.0), Lc((size_t)p * p, 0.0), w(p), y(p);
    double gmax = 0.0;
    for (int i = 0; i < p; ++i)
      for (int j = 0; j < p; ++j) { double t = 0.0; for (int c = 0; c < D; ++c) t += A[i + (size_t)p * c] * A[j + (size_t)p * c]; G[i + (size_t)p * j] = t; if (i == j) gmax = std::fmax(gmax, t); }
    for (int j = 0; j < p; ++j) {  // Cholesky of A A'
      double d = G[j + (size_t)p * j];
      for (int k = 0; k < j; ++k) d -= Lc[j + (size_t)p * k] * Lc[j + (size_t)p * k];
      if (!(d > 1e-12 * gmax)) return fail(TO_ERR_UNSUPPORTED, "per-trajectory b of a LinearConstraint: the rows of A must be linearly independent");
      Lc[j + (size_t)p * j] = std::sqrt(d);
      for (int i = j + 1; i < p; ++i) {
        double t = G[i + (size_t)p * j];
        for (int k = 0; k < j; ++k) t -= Lc[i + (size_t)p * k] * Lc[j + (size_t)p * k];
        Lc[i + (size_t)p * j] = t / Lc[j + (size_t)p * j];
      }
    }
    for (int b = 0; b < B; ++b) {
      for (int i = 0; i < p; ++i) { double t = params[i + (size_t)p * b] - b0[i]; for (int k = 0; k < i; ++k) t -= Lc[i + (size_t)p * k] * y[k]; y[i] = t / Lc[i + (size_t)p * i]; }
      for (int i = p - 1; i >= 0; --i) { double t = y[i]; for (int k = i + 1; k < p; ++k) t -= Lc[k + (size_t)p * i] * w[k]; w[i] = t / Lc[i + (size_t)p * i]; }
      for (int c = 0; c < D; ++c) { double t = 0.0; for (int i = 0; i < p; ++i) t += A[i + (size_t)p * c] * w[i]; shift[(size_t)(ci.d.inds[c] - 1) + (size_t)nz * b] += t; }
    }
  }
  shift_out->swap(shift);
  return TO_OK;
}

// to_set_cost_linear_batch (DevProblem::gl): q[n, B] / r[m, B] as the difference from the descriptor's, which the kernels ADD to the shared
// terms; a NULL argument leaves its output alone.  cost_linear_zero: the rows [n + m, B] a cost starts over with behind to_set_cost.
inline int cost_linear_delta(const to_cost_desc& c, int n, int m, int B, const double* q, const double* r, std::vector<double>* dq, std::vector<double>* dr) {
  if (!q && !r) return fail(TO_ERR_NULL, "null pointer");
  if (c.kind == TO_COST_ERROR_QUADRATIC) return fail(TO_ERR_UNSUPPORTED, "per-trajectory linear terms: not for ErrorQuadratic (its q slot carries x_ref)");
  if (q) {
    dq->resize((size_t)n * B);
    for (int b = 0; b < B; ++b) for (int i = 0; i < n; ++i) (*dq)[i + (size_t)n * b] = q[i + (size_t)n * b] - c.q[i];
  }
  if (r) {
    dr->resize((size_t)m * B);
    for (int b = 0; b < B; ++b) for (int j = 0; j < m; ++j) (*dr)[j + (size_t)m * b] = r[j + (size_t)m * b] - c.r[j];
  }
  return TO_OK;
}
inline void cost_linear_zero(int n, int m, int B, std::vector<double>* rows) { rows->assign((size_t)(n + m) * B, 0.0); }

// THE rule for a second set of model parameters pp[16] next to the problem's mp (model_key as in TrackFacts): the entries that select dimensions
// or the attitude representation must be equal.  Key 8 (model vector) takes no such set.  (to_set_model_params_batch never gets here with a key
// above 4: plants_supported refuses first.)
inline bool all_finite(const double* v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }
inline bool plant_params_compatible(int key, const double* mp, const double* pp) {
  auto same = [&](int i) { return pp[i] == mp[i]; };
  if (key == 8) return false;
  if (key <= 2 || key == 7) return same(1);         // double integrator: D; hybrid double integrator: S
  if (key >= 4 && key <= 6) return same(10);        // Quadrotor: rotation
  if (key == 9 || key == 10) return same(15) && same(1);  // InfeasibleModel: the base model, and its D
  if (key == 11) return same(15);
  return true;
}
// The refusal of one set.  need_finite: a plant the problem is PLANNED on (to_set_model_params_batch: "the parameters", every entry finite); else
// one a rollout simulates ("plant_params").  where: "" or " of <which one>"; a caller with many sets asks the predicates first and formats once.
inline int validate_plant_params(const char* who, int key, const double* mp, const double* pp, bool need_finite, const std::string& where) {
  if (key == 8) return fail(TO_ERR_ARGUMENT, std::string(who) + ": a model vector takes no plant_params (its models live in the step table)");
  for (int i = 0; need_finite && i < 16; ++i)
    if (!std::isfinite(pp[i])) return fail(TO_ERR_ARGUMENT, std::string(who) + ": entry " + std::to_string(i) + where + " is not finite");
  if (!plant_params_compatible(key, mp, pp))
    return fail(TO_ERR_ARGUMENT, std::string(who) + ": " + (need_finite ? "the parameters" : "plant_params") + where +
                                     " change the model's dimensions or attitude representation");
  return TO_OK;
}

}  // namespace to
