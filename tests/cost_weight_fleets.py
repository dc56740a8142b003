"""Fleets for per-trajectory cost weights (to_set_cost_weights_batch; tests/test_cost_weight_fleets_oracle.py vets them on the CPU,
tests/test_gpu_cost_weights.py holds the HIP library to them).  The reference is B single-trajectory ORACLE problems, problem b built with
trajectory b's own diagonal Q / R in its cost descriptors and — through ``batch=1, b_offset=b`` — its own start state (the scheme of
tests/constraint_limit_fleets.py).  The oracle knows nothing about per-trajectory weights and is not changed.  Every draw comes from a
seeded generator; a reference is computed once per session and shared, and nothing in it is modified afterwards.

Every weight is the nominal one times 10^U(-0.5, 0.5), drawn per trajectory AND per entry: a decade of spread, and no two entries of a
trajectory scaled alike, so that a kernel reading a neighbouring row or another trajectory's column is seen.  A single is built with
q = -Q_b xf, r = -R_b uf and the NOMINAL constant c — what ``set_LQR_weights_batch`` leaves on the batch (``set_LQR_goal!`` does not
touch c either), so that costs compare as well as trajectories.

  cartpole         Cartpole N = 41, tf = 2, B = 70 (two tiles, the second partial) and B = 300 (the lane path with compaction);
                   nominal Q = 1e-2, R = 1e-1, Qf = 100
  dint             2-D double integrator N = 51, tf = 5, B = 40, goal [1, 2, 0, 0]; nominal Q = 1, R = 0.1, Qf = 100; x0[:2] ~ U(-0.2, 0.2)
  quadrotor        Quadrotor with DiagonalQuatCost (configs.quadrotor_problem's QuatLQRCost pair), N = 31, tf = 1, B = 24
  cartpole_knots   Cartpole N = 41, tf = 2, B = 70 with a distinct cost per knot (n_costs = N), every knot's weights drawn on their own
Variants: ``free`` (no constraints; iLQR) and ``bound`` (a control bound on knots 1 .. N-1; AL with constraint_tolerance 1e-4 and ALTRO).
"""
import math
from types import SimpleNamespace

import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

OK = T.capi.SOLVE_SUCCEEDED
AL_KW = dict(constraint_tolerance=1e-4)
STAT_KEYS = ("iterations", "iterations_outer", "iterations_pn", "status", "cost", "c_max")
SOLVERS = {"ilqr": (T.iLQRSolver, {}), "al": (T.ALSolver, AL_KW), "altro": (T.ALTROSolver, {})}
DINT_XF = np.array([1.0, 2.0, 0.0, 0.0])
U_BOUND = {"cartpole": 6.0, "cartpole_knots": 6.0, "dint": 1.5, "quadrotor": 3.0}   # |u| <= bound (Quadrotor: 0 <= u <= bound)
SEEDS = {("cartpole", 70): 301, ("cartpole", 300): 302, ("dint", 40): 303, ("quadrotor", 24): 304, ("cartpole_knots", 70): 305}
# X / U tolerance of the solves in assert_trajectories_close's measure, per (fleet, B, variant, solver) where the default — 1e-6, 1e-5 for AL,
# the bounds of tests/test_gpu_constraint_limits.py::test_solves and tests/test_goal_batch.py — is below the oracle's own +-1-ulp spread
# (tests/test_cost_weight_fleets_oracle.py measures it; the margin is that of tests/test_oracle_sensitivity.py)
SOLVE_RTOL = {}


def spread(rng, shape):
    return 10.0 ** rng.uniform(-0.5, 0.5, shape)


# ------------------------------------------------------------------------------------------------ nominal problems
def _cartpole_nominal():
    return np.full(4, 1e-2), np.full(1, 1e-1), np.full(4, 100.0), np.array([0.0, math.pi, 0.0, 0.0]), np.zeros(1)


def _quadrotor_nominal():
    th = math.radians(135.0) / 2
    xf = np.zeros(13)
    xf[:3] = [2.0, 3.0, 1.0]
    xf[3:7] = [math.cos(th), 0.0, 0.0, math.sin(th)]
    Qd = np.array([1.0, 1, 1, 0, 0, 0, 0, .1, .1, .1, .1, .1, .1])
    return Qd, np.full(4, 1e-2), 100.0 * Qd, xf, T.Quadrotor().hover_control()


def _diag_costs(Q, R, Qf, xf, uf, Q0, R0, Qf0, quat=False):
    """(stage, terminal) cost objects with weights Q, R, Qf, linear terms for the goal (xf, uf) and the constants of the NOMINAL weights."""
    c0 = 0.5 * xf @ (Q0 * xf) + 0.5 * uf @ (R0 * uf)
    cf0 = 0.5 * xf @ (Qf0 * xf) + (0.5 * uf @ (R0 * uf) if quat else 0.0)
    if quat:
        q_ref = xf[3:7]
        return (T.DiagonalQuatCost(Q, R, -Q * xf, -R * uf, c0, 1.0, q_ref),
                T.DiagonalQuatCost(Qf, R, -Qf * xf, -R * uf, cf0, 1.0, q_ref, terminal=True))
    return T.DiagonalCost(Q, R, -Q * xf, -R * uf, c0), T.DiagonalCost(Qf, R, -Qf * xf, -R * uf, cf0, terminal=True)


class Spec:
    """One fleet: ``single(lib, b, variant)`` — trajectory b's own problem, its weights in the descriptors; ``shared(lib, variant)`` — the
    batch on the nominal weights; ``set_weights(p)`` — the per-trajectory weights onto such a batch; ``Q`` [B, n_costs, n], ``R``
    [B, n_costs, m]: the weights of every distinct cost (stage, terminal — or one per knot)."""

    def __init__(self, name, B):
        self.name, self.B = name, B
        rng = np.random.default_rng(SEEDS[name, B])
        if name.startswith("cartpole"):
            self.N, self.tf = 41, 2.0
            self.Q0, self.R0, self.Qf0, self.xf, self.uf = _cartpole_nominal()
        elif name == "dint":
            self.N, self.tf = 51, 5.0
            self.Q0, self.R0, self.Qf0, self.xf, self.uf = np.ones(4), 0.1 * np.ones(2), 100 * np.ones(4), DINT_XF, np.zeros(2)
            self.x0 = np.zeros((B, 4))
            self.x0[:, :2] = rng.uniform(-0.2, 0.2, (B, 2))
        elif name == "quadrotor":
            self.N, self.tf = 31, 1.0
            self.Q0, self.R0, self.Qf0, self.xf, self.uf = _quadrotor_nominal()
        else:
            raise ValueError(name)
        self.n, self.m = self.Q0.size, self.R0.size
        self.n_costs = self.N if name == "cartpole_knots" else 2
        nc = self.n_costs
        self.Q = np.empty((B, nc, self.n)); self.R = np.empty((B, nc, self.m))
        self.Q[:, :-1] = self.Q0 * spread(rng, (B, nc - 1, self.n))
        self.Q[:, -1] = self.Qf0 * spread(rng, (B, self.n))
        self.R[:] = self.R0 * spread(rng, (B, nc, self.m))
        if nc == 2:
            self.R[:, 1] = self.R[:, 0]              # LQRObjective: the terminal cost carries the stage R

    # ---- problems
    def _objective(self, Q, R):
        """Q [n_costs, n], R [n_costs, m] -> Objective"""
        quat = self.name == "quadrotor"
        if self.n_costs == 2:
            stage, term = _diag_costs(Q[0], R[0], Q[1], self.xf, self.uf, self.Q0, self.R0, self.Qf0, quat)
            return T.Objective(stage, term, self.N)
        costs = [_diag_costs(Q[k], R[k], Q[k], self.xf, self.uf, self.Q0, self.R0, self.Qf0)[0] for k in range(self.N - 1)]
        costs.append(_diag_costs(Q[-1], R[-1], Q[-1], self.xf, self.uf, self.Q0, self.R0, self.Qf0)[1])
        return T.Objective(costs)

    def _nominal_weights(self):
        Q = np.tile(self.Q0, (self.n_costs, 1)); Q[-1] = self.Qf0
        return Q, np.tile(self.R0, (self.n_costs, 1))

    def _problem(self, lib, batch, b_offset, Q, R, variant):
        n, m, N = self.n, self.m, self.N
        cons = T.ConstraintList(n, m, N)
        if variant == "bound":
            ub = U_BOUND[self.name]
            T.add_constraint(cons, T.BoundConstraint(n, m, u_min=0.0 if self.name == "quadrotor" else -ub, u_max=ub), range(1, N))
        elif variant != "free":
            raise ValueError(variant)
        if self.name.startswith("cartpole"):
            model, x0, U0 = T.Cartpole(), configs.cartpole_x0(batch, b_offset), np.full(m, 0.01)
        elif self.name == "dint":
            model, x0, U0 = T.DoubleIntegrator(1.0, 2), self.x0[b_offset:b_offset + batch], np.zeros(m)
        else:
            model, x0, U0 = T.Quadrotor(), configs.quadrotor_x0(batch, b_offset), T.Quadrotor().hover_control()
        p = T.Problem(model, self._objective(Q, R), np.zeros(n), self.tf, xf=self.xf, constraints=cons, batch=batch, lib=lib)
        p.set_initial_state(x0)
        T.initial_controls(p, U0)
        return p

    def single(self, lib, b, variant="free"):
        return self._problem(lib, 1, b, self.Q[b], self.R[b], variant)

    def shared(self, lib, variant="free", batch=None, b_offset=0):
        return self._problem(lib, self.B if batch is None else batch, b_offset, *self._nominal_weights(), variant)

    def set_weights(self, p, sel=None):
        """The fleet's weights (of the trajectories ``sel``; default all) onto a batch on nominal weights, with the goal's linear terms."""
        sel = np.arange(self.B) if sel is None else np.asarray(sel)
        for ci in range(self.n_costs):
            Q, R = np.ascontiguousarray(self.Q[sel, ci]), np.ascontiguousarray(self.R[sel, ci])
            T.set_cost_weights_batch(p, ci, Q=Q, R=R)
            q, r = np.ascontiguousarray(-Q * self.xf), np.ascontiguousarray(-R * self.uf)
            p._call("set_cost_linear_batch", ci, p._pd(q), p._pd(r))

    def batch(self, lib, variant="free"):
        p = self.shared(lib, variant)
        self.set_weights(p)
        return p


def phases(p):
    """Everything the phase comparison looks at, after a rollout (and two dual updates where there are constraints)."""
    T.rollout(p)
    if len(p.constraints):
        I.dual_update(p); I.dual_update(p)
    r = SimpleNamespace(J=T.cost(p), Jk=T.stage_costs(p), al=I.al_cost(p) if len(p.constraints) else T.cost(p))
    r.grad, r.hess = I.cost_gradient_hessian(p)                      # to_cost_expansion: the objective alone, full state
    I.expand(p)
    e = I.cost_expansion(p)                                          # to_get_cost_expansion: cost + AL blocks on the error state
    r.E = np.concatenate([np.asarray(e[k]).reshape(p.B, -1) for k in ("Qxx", "Quu", "Qux", "qx", "qu")], axis=1)
    I.backwardpass(p)
    g = I.gains(p)
    r.K, r.d = g["K"], g["d"]
    r.ls, r.Jn = I.forwardpass(p)
    return r


def _stack(rows):
    out = SimpleNamespace()
    for k in vars(rows[0]):
        setattr(out, k, np.concatenate([np.asarray(getattr(r, k)) for r in rows], axis=0))
    return out


_cache = {}


def spec(name, B):
    if ("spec", name, B) not in _cache:
        _cache["spec", name, B] = Spec(name, B)
    return _cache["spec", name, B]


def reference_phases(name, B, variant, oracle):
    key = ("phases", name, B, variant)
    if key not in _cache:
        s = spec(name, B)
        _cache[key] = _stack([phases(s.single(oracle, b, variant)) for b in range(B)])
    return _cache[key]


def solve_singles(problems, Solver, kw):
    stats, X, U = {k: [] for k in STAT_KEYS}, [], []
    for p in problems:
        st = Solver(p, **kw).solve().stats
        for k in STAT_KEYS:
            stats[k].append(st[k][0])
        X.append(T.states(p)[0]); U.append(T.controls(p)[0])
    stats = {k: np.array(v) for k, v in stats.items()}
    return SimpleNamespace(B=len(X), stats=stats, X=np.array(X), U=np.array(U), total_iterations=int(stats["iterations"].sum()))


def variant_of(solver):
    return "free" if solver == "ilqr" else "bound"


def reference_solve(name, B, solver, oracle):
    """The B singles solved with ``solver`` ("ilqr" on the free variant, "al" / "altro" on the bound one), stacked."""
    key = ("solve", name, B, solver)
    if key not in _cache:
        s = spec(name, B)
        Solver, kw = SOLVERS[solver]
        _cache[key] = solve_singles([s.single(oracle, b, variant_of(solver)) for b in range(B)], Solver, kw)
    return _cache[key]


def ulp_moved(p, ulps):
    """The problem with its start state and control guess moved by ``ulps`` units in the last place (towards +inf; negative: -inf)."""
    to = np.inf if ulps > 0 else -np.inf
    x0, U = p.x0.copy(), T.controls(p)
    for _ in range(abs(ulps)):
        x0, U = np.nextafter(x0, to), np.nextafter(U, to)
    p.set_initial_state(x0)
    T.initial_controls(p, U)
    return p


def ulp_solve(name, B, solver, oracle, ulps):
    """The B singles solved from inputs moved by +-1 ulp: what the oracle's own integers and answers do under a change of rounding."""
    key = ("ulp", name, B, solver, ulps)
    if key not in _cache:
        s = spec(name, B)
        Solver, kw = SOLVERS[solver]
        _cache[key] = solve_singles([ulp_moved(s.single(oracle, b, variant_of(solver)), ulps) for b in range(B)], Solver, kw)
    return _cache[key]


def shared_solve(name, B, solver, oracle):
    """The same fleet on the nominal weights for every trajectory (one oracle batch)."""
    key = ("shared", name, B, solver)
    if key not in _cache:
        s = spec(name, B)
        Solver, kw = SOLVERS[solver]
        p = s.shared(oracle, variant_of(solver))
        st = Solver(p, **kw).solve().stats
        _cache[key] = SimpleNamespace(stats={k: st[k].copy() for k in STAT_KEYS}, X=T.states(p), U=T.controls(p))
    return _cache[key]


def relerr(A, R):
    A, R = A.reshape(A.shape[0], -1), R.reshape(R.shape[0], -1)
    return np.abs(A - R).max(axis=1) / np.maximum(1.0, np.abs(R).max(axis=1))


def solve_rtol(name, B, solver):
    return SOLVE_RTOL.get((name, B, solver), 1e-5 if solver == "al" else 1e-6)


# ------------------------------------------------------------------------------------------------ combination: weights + goals + limits + plants + steps
COMBO_B, COMBO_N, COMBO_TF = 24, 41, 2.0


def combo(B=COMBO_B):
    """Cartpole with weights, goals (the costs' linear terms), control bounds, plants and time steps all per trajectory:
    -> SimpleNamespace(Q, R, Qf [B, .], Xf [B, 4], u_max [B], models [B], dt [B, N-1])."""
    if "combo" not in _cache:
        import model_params_fleet as MF
        rng = np.random.default_rng(311)
        Q0, R0, Qf0, xf, _ = _cartpole_nominal()
        Xf = np.tile(xf, (B, 1)); Xf[:, 0] += rng.uniform(-0.3, 0.3, B)
        tf = COMBO_TF * rng.uniform(0.85, 1.15, B)
        _cache["combo"] = SimpleNamespace(Q=Q0 * spread(rng, (B, 4)), R=R0 * spread(rng, (B, 1)), Qf=Qf0 * spread(rng, (B, 4)), Xf=Xf,
                                          u_max=rng.uniform(5.0, 8.0, B), models=MF.draw_models("cartpole", B, 312, spread=0.1),
                                          dt=np.repeat(tf[:, None] / (COMBO_N - 1), COMBO_N - 1, axis=1))
    return _cache["combo"]


def _combo_problem(lib, batch, b_offset, Q, R, Qf, xf, u_max, model=None, dt=None):
    Q0, R0, Qf0, xf0, uf = _cartpole_nominal()
    c0, cf0 = 0.5 * xf0 @ (Q0 * xf0), 0.5 * xf0 @ (Qf0 * xf0)              # the constants of the nominal descriptors: no setter touches c
    obj = T.Objective(T.DiagonalCost(Q, R, -Q * xf, -R * uf, c0), T.DiagonalCost(Qf, R, -Qf * xf, -R * uf, cf0, terminal=True), COMBO_N)
    cons = T.ConstraintList(4, 1, COMBO_N)
    T.add_constraint(cons, T.BoundConstraint(4, 1, u_min=-u_max, u_max=u_max), range(1, COMBO_N))
    p = T.Problem(model if model is not None else T.Cartpole(), obj, np.zeros(4), COMBO_TF if dt is None else float(np.sum(dt)), xf=xf, constraints=cons,
                  batch=batch, lib=lib, dt=dt)
    p.set_initial_state(configs.cartpole_x0(batch, b_offset))
    T.initial_controls(p, np.full(1, 0.01))
    return p


def combo_single(lib, b):
    c = combo()
    return _combo_problem(lib, 1, b, c.Q[b], c.R[b], c.Qf[b], c.Xf[b], c.u_max[b], c.models[b], c.dt[b])


def combo_shared(lib):
    Q0, R0, Qf0, xf, _ = _cartpole_nominal()
    return _combo_problem(lib, COMBO_B, 0, Q0, R0, Qf0, xf, 6.0)


COMBO_SETTERS = ("weights", "limits", "plants", "steps")


def combo_apply(p, order=COMBO_SETTERS):
    c = combo()
    for what in order:
        if what == "weights":
            T.set_LQR_weights_batch(p, c.Q, c.R, c.Qf, xf=c.Xf)            # weights AND the goals' linear terms (gl)
        elif what == "limits":
            T.set_bounds_batch(p, 0, u_max=c.u_max[:, None], u_min=-c.u_max[:, None])
        elif what == "plants":
            T.set_model_params(p, c.models)
        else:
            T.set_time_steps_batch(p, c.dt)
    return p


def combo_reference(oracle, solver="altro", ulps=0):
    key = ("combo", solver, ulps)
    if key not in _cache:
        Solver, kw = SOLVERS[solver]
        ps = [combo_single(oracle, b) for b in range(COMBO_B)]
        _cache[key] = solve_singles([ulp_moved(q, ulps) if ulps else q for q in ps], Solver, kw)
    return _cache[key]
