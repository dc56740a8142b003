"""Reference for per-trajectory model parameters (tests/test_gpu_model_params_batch.py, tests/test_gpu_model_params_instances.py): B
single-trajectory ORACLE problems, problem b built with its own model and — through ``batch=1, b_offset=b`` — with trajectory b's own start state (the scheme of
tests/test_goal_batch.py).  The oracle itself knows nothing about per-trajectory parameters and is not changed.  A fleet is computed once
per configuration and shared by the tests that need it (``fleet``); nothing in it is modified afterwards."""
from types import SimpleNamespace

import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

SPREAD = 0.2  # parameters within +-20 % of the configuration's values


def dint_dim(kind, D=None):
    """The dimension of a double-integrator kind: ``dintD_con`` names its own, ``dint`` takes the argument (default 2)."""
    if kind.startswith("dint") and kind.endswith("_con"):
        return int(kind[4])
    return 2 if D is None else int(D)


def draw_models(kind, B, seed, spread=SPREAD, D=None):
    """B models of the problem's class, parameters drawn uniformly within +-spread of the nominal ones by a seeded generator; model 0 keeps
    the nominal (shared) values.  Cartpole: cart mass, pole mass, pole length; Quadrotor: mass, the three inertias, the torque constant
    km; double integrator (``D`` dimensions): the mass.  (Gravity, the motor geometry and the entries that select dimensions stay the
    problem's.)"""
    rng = np.random.default_rng(seed)
    f = lambda k: 1.0 + spread * rng.uniform(-1.0, 1.0, (B, k))
    if kind.startswith("cartpole"):
        s = f(3)
        models = [T.Cartpole(mc=1.0 * a, mp=0.2 * b, l=0.5 * c) for a, b, c in s]
        models[0] = T.Cartpole()
    elif kind.startswith("quadrotor"):
        s = f(5)
        models = [T.Quadrotor(mass=0.5 * a, J=(0.0023 * b, 0.0023 * c, 0.004 * d), km=0.0245 * e) for a, b, c, d, e in s]
        models[0] = T.Quadrotor()
    elif kind.startswith("dint"):
        D = dint_dim(kind, D)
        s = f(1)
        models = [T.DoubleIntegrator(1.0 * a, D) for (a,) in s]
        models[0] = T.DoubleIntegrator(1.0, D)
    else:
        raise ValueError(kind)
    return models


def params_of(models):
    pp = np.zeros((len(models), 16))
    for b, mod in enumerate(models):
        q = mod.params()
        pp[b, : len(q)] = q
    return pp


def build(kind, lib, batch, b_offset=0, model=None, N=None, tf=None, x0=None, integration=T.RK4, D=None, options=None):
    """The problem of a configuration on ``lib``; ``model``: the model it is built on (default: the nominal one); ``x0``: one start state for
    every trajectory instead of the configuration's per-trajectory ones; ``integration``: the integrator; ``D``: the dimension of the
    double integrator ``dint``; ``options``: keywords of the problem's ``SolverOptions``.

    ``quadrotor_con``: the constrained Quadrotor with the goal on position and velocities.  ``dintD_con`` (D = 1, 2, 3): |u| <= 1.5 on knots
    1 .. N-1 and a GoalConstraint at N, xf = [0.5 (1 .. D), 0 ...] — with xf = (1, 2, 3) the bound puts the goal out of reach of the heavier
    plants of D = 3 (79 % of a fleet succeed on the oracle); N = 31, tf = 3.  ``dint_free``: ``dint`` without its bounds (the unconstrained
    forward variants)."""
    kw = dict(batch=batch, b_offset=b_offset, lib=lib, model=model, integration=integration)
    if options:
        kw["options"] = T.SolverOptions(lib=lib, **options)
    if kind == "cartpole":
        p = configs.cartpole_problem(N=N or 31, tf=tf or 1.5, **kw)
    elif kind == "cartpole_con":
        p = configs.cartpole_problem(N=N or 51, tf=tf or 2.5, constrained=True, u_bnd=10.0, **kw)
    elif kind == "quadrotor":
        p = configs.quadrotor_problem(N=N or 41, tf=tf or 1.0, **kw)
    elif kind == "quadrotor_con":
        p = configs.quadrotor_problem(N=N or 31, tf=tf or 2.5, constrained=True, goal_inds=configs.C5_GOAL_INDS, **kw)
    elif kind.startswith("dint"):
        con = kind.endswith("_con")
        D = dint_dim(kind, D)
        n, m, Nn = 2 * D, D, N or 31
        mdl = model if model is not None else T.DoubleIntegrator(1.0, D)
        xf = np.r_[(0.5 if con else 1.0) * np.arange(1, D + 1), np.zeros(D)]
        obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 100 * np.ones(n), xf, Nn)
        cons = T.ConstraintList(n, m, Nn)
        if kind != "dint_free":
            T.add_constraint(cons, T.BoundConstraint(n, m, u_max=1.5, u_min=-1.5), (1, Nn - 1))
        if con:
            T.add_constraint(cons, T.GoalConstraint(xf), Nn)
        p = T.Problem(mdl, obj, np.zeros(n), tf or 3.0, xf=xf, constraints=cons, batch=batch, lib=lib, integration=integration,
                      **({"options": kw["options"]} if options else {}))
        b = np.arange(b_offset, b_offset + batch, dtype=np.uint64)
        X0 = np.zeros((batch, n))
        for j in range(D):
            X0[:, j] = configs.splitmix64_uniform(7, np.uint64(D) * b + np.uint64(j)) - 0.5
        p.set_initial_state(X0)
    else:
        raise ValueError(kind)
    if x0 is not None:
        p.set_initial_state(np.tile(np.asarray(x0, dtype=np.float64), (batch, 1)))
    return p


SOLVERS = {"ilqr": T.iLQRSolver, "al": T.ALSolver, "altro": T.ALTROSolver}


def phase_loop(p, iters=30, dual_every=10):
    """``iters`` rounds of expand / backward pass / forward pass from the rolled-out start, a dual update ahead of every ``dual_every``-th:
    -> (line-search indices [iters, B], J_new [iters, B], X, U)."""
    T.rollout(p)
    ls, Jn = [], []
    for it in range(iters):
        if it % dual_every == dual_every - 1:
            I.dual_update(p)
        I.expand(p); I.backwardpass(p)
        l, J = I.forwardpass(p)
        ls.append(l); Jn.append(J)
    return np.array(ls), np.array(Jn), T.states(p), T.controls(p)


class Fleet:
    """Results of B single-trajectory oracle problems, stacked along the batch axis."""

    def __init__(self, kind, oracle, models, solver=None, phases=False, x0=None, sel=None, goals=None, loop=0, solver_kw=None, **kw):
        """``sel``: the trajectories to run (default: all of them), e.g. a sample of a large batch; ``goals``: [B, n], problem b is
        retargeted with the scalar ``set_goal_state(p, goals[b])``; ``loop``: rounds of ``phase_loop`` (-> ls_loop, Jn_loop [rounds, B],
        X_loop, U_loop); ``solver_kw``: keywords of the solver."""
        sel = range(len(models)) if sel is None else sel
        self.B = len(sel)
        keys = ("iterations", "iterations_outer", "iterations_pn", "status", "cost", "c_max")
        self.stats = {k: [] for k in keys}
        rows = {k: [] for k in ("X", "U", "Xr", "J", "F", "A", "Bm", "K", "d", "ls", "Jn", "defect", "ls_loop", "Jn_loop", "X_loop", "U_loop")}
        for b in sel:
            p = build(kind, oracle, 1, b_offset=int(b), model=models[b], x0=x0, **kw)
            if goals is not None:
                T.set_goal_state(p, np.asarray(goals)[b])
            if loop:
                l, J, X, U = phase_loop(p, loop)
                rows["ls_loop"].append(l[:, 0]); rows["Jn_loop"].append(J[:, 0]); rows["X_loop"].append(X[0]); rows["U_loop"].append(U[0])
                continue
            if phases:
                T.rollout(p)
                rows["Xr"].append(T.states(p)[0]); rows["J"].append(T.cost(p)[0])
                rows["F"].append(I.discrete_jacobian(p)[0])
                rows["defect"].append(T.dynamics_defect(p)[0])
                I.expand(p)
                A, Bm = I.dynamics_jacobians(p)
                rows["A"].append(A[0]); rows["Bm"].append(Bm[0])
                I.backwardpass(p)
                g = I.gains(p)
                rows["K"].append(g["K"][0]); rows["d"].append(g["d"][0])
                ls, Jn = I.forwardpass(p)
                rows["ls"].append(ls[0]); rows["Jn"].append(Jn[0])
            if solver:
                s = SOLVERS[solver](p, **(solver_kw or {})).solve()
                for k in keys:
                    self.stats[k].append(s.stats[k][0])
                rows["X"].append(T.states(p)[0]); rows["U"].append(T.controls(p)[0])
        self.stats = {k: np.array(v) for k, v in self.stats.items() if v}
        for k, v in rows.items():
            if v:
                setattr(self, k, np.array(v))
        if loop:
            self.ls_loop, self.Jn_loop = self.ls_loop.T, self.Jn_loop.T                # [rounds, B], as phase_loop returns them
        if solver:
            self.total_iterations = int(self.stats["iterations"].sum())


_cache = {}


def _hashable(v):
    if isinstance(v, dict):
        return tuple(sorted((k, _hashable(x)) for k, x in v.items()))
    if isinstance(v, np.ndarray):
        return (v.shape, v.tobytes())
    return v


def fleet(kind, oracle, B, seed, solver=None, phases=False, x0=None, sel=None, **kw):
    """The fleet of a configuration, computed once per session."""
    key = (kind, B, seed, solver, phases, None if x0 is None else tuple(x0), None if sel is None else tuple(sel),
           tuple(sorted((k, _hashable(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = Fleet(kind, oracle, draw_models(kind, B, seed, D=kw.get("D")), solver=solver, phases=phases, x0=x0, sel=sel, **kw)
    return _cache[key]


def assert_fleet_parity(sh, ph, fl, rtol=1e-6, unconverged_rtol=None, sel=None):
    """tests/test_gpu_parity.py assert_solve_parity with a fleet in the oracle batch's place (``sel``: the trajectories of ``ph`` the fleet
    holds, in its order): integer outputs equal; cost rtol 1e-8 (the per-trajectory tests' bound); X / U within rtol in that function's
    measure (largest deviation of a trajectory against max(1, its largest entry)) — the trajectories the oracle itself cut off at an
    iteration limit within unconverged_rtol."""
    from test_gpu_parity import assert_trajectories_close
    sel = np.arange(ph.B) if sel is None else np.asarray(sel)
    for k in ("iterations", "iterations_outer", "status"):
        np.testing.assert_array_equal(sh.stats[k][sel], fl.stats[k], err_msg=k)
    np.testing.assert_allclose(sh.stats["cost"][sel], fl.stats["cost"], rtol=1e-8)
    np.testing.assert_allclose(sh.stats["c_max"][sel], fl.stats["c_max"], rtol=1e-3, atol=1e-9)
    done = (fl.stats["status"] == T.capi.SOLVE_SUCCEEDED) if unconverged_rtol else np.ones(len(sel), bool)
    tol = np.where(done, rtol, unconverged_rtol or rtol)
    assert_trajectories_close(T.states(ph)[sel], fl.X, tol, "X")
    assert_trajectories_close(T.controls(ph)[sel], fl.U, tol, "U")


# ------------------------------------------------------------------------------------------------ the named fleets
def cartpole_goal_fleet(B, con=False):
    """One goal per trajectory: tests/test_goal_batch.py cartpole_goals (halved cart positions under a GoalConstraint, as there)."""
    from test_goal_batch import cartpole_goals
    Xf = cartpole_goals(B, seed=3 if con else 5)
    if con:
        Xf[:, 0] *= 0.5
    return Xf


def quadrotor_goal_fleet(B):
    """tests/test_goal_batch.py's Quadrotor goals: the configuration's goal with the position moved by up to 0.5 m per axis."""
    th = np.radians(135.0) / 2
    Xf = np.tile(np.r_[2.0, 3.0, 1.0, np.cos(th), 0.0, 0.0, np.sin(th), np.zeros(6)], (B, 1))               # configs.quadrotor_problem's xf
    Xf[:, :3] += np.random.default_rng(8).uniform(-0.5, 0.5, (B, 3))
    return Xf


QUAD = dict(N=31, tf=1.0)
ALTRO_Q = dict(n_steps=configs.C5_PN_STEPS)
# The fleets of tests/test_gpu_model_params_instances.py, every one vetted on the oracle alone by tests/test_model_params_fleets_oracle.py
# before its seed was fixed.  name: (kind, B, seed, solver, keywords of Fleet / build)
FLEETS = {
    # a. run-time integrator instances
    "cartpole_rk3": ("cartpole", 70, 81, "ilqr", dict(integration=T.RK3)),
    "cartpole_euler": ("cartpole", 70, 82, "ilqr", dict(integration=T.Euler)),
    "dint_rk3": ("dint", 70, 83, "al", dict(integration=T.RK3)),
    "dint_euler": ("dint", 70, 84, "al", dict(integration=T.Euler)),
    "quadrotor_rk3": ("quadrotor", 70, 85, "ilqr", dict(integration=T.RK3, **QUAD)),
    "quadrotor_euler": ("quadrotor", 70, 86, "ilqr", dict(integration=T.Euler, **QUAD)),
    "cartpole_con_rk3": ("cartpole_con", 70, 87, "altro", dict(integration=T.RK3)),
    # b. every dimension of the double integrator
    "dint1_con": ("dint1_con", 70, 91, "altro", {}),
    "dint2_con": ("dint2_con", 70, 92, "altro", {}),
    "dint3_con": ("dint3_con", 70, 93, "altro", {}),
    # c. Cartpole on the tangent-matrix layout
    "cartpole_rk4": ("cartpole", 70, 11, "ilqr", {}),
    "cartpole_con_al": ("cartpole_con", 70, 14, "al", {}),
    # e. Quadrotor ALTRO
    "quadrotor_con": ("quadrotor_con", 70, 94, "altro", dict(solver_kw=ALTRO_Q)),
    # f. plants together with per-trajectory goals
    "cartpole_goals": ("cartpole", 70, 95, "ilqr", dict(goals=cartpole_goal_fleet(70))),
    "quadrotor_goals": ("quadrotor", 70, 96, "ilqr", dict(goals=quadrotor_goal_fleet(70), **QUAD)),
    "cartpole_con_goals": ("cartpole_con", 70, 97, "altro", dict(goals=cartpole_goal_fleet(70, con=True))),
}
POLISHED = ("cartpole_con_rk3", "dint1_con", "dint2_con", "dint3_con", "quadrotor_con", "cartpole_con_goals")
# d. deep line searches: the phase loop on the constrained Quadrotor
DEEP = ("quadrotor_con", 44, 98, dict(N=41, tf=3.0, options=dict(constraint_tolerance=1e-4), loop=30))


def named_fleet(name, oracle, phases=False):
    """The solve fleet of FLEETS[name], or its phases fleet."""
    kind, B, seed, solver, kw = FLEETS[name]
    return fleet(kind, oracle, B, seed, solver=None if phases else solver, phases=phases, **kw)


def build_kw(kw):
    """The keywords of a FLEETS entry that ``build`` takes."""
    return {k: v for k, v in kw.items() if k not in ("goals", "loop", "solver_kw")}


LINEAR_SEED = 88
_linear = {}


def linear_fleet(oracle, B, seed):
    """tests/test_goal_batch.py linear_problem, problem b rebuilt on model b with right-hand side b in its descriptor."""
    from test_goal_batch import linear_problem, linear_rhs
    if (B, seed) not in _linear:
        models, bv = draw_models("dint", B, seed), linear_rhs(B)
        x0 = linear_problem(oracle, B)[1]
        keys = ("iterations", "iterations_outer", "iterations_pn", "status", "cost", "c_max")
        stats, X, U = {k: [] for k in keys}, [], []
        for b in range(B):
            p1, _ = linear_problem(oracle, 1)
            p1.constraints.constraints[0].b = bv[b].copy()
            q = T.Problem(models[b], p1.obj, x0[b], 3.0, xf=p1.xf, constraints=p1.constraints, batch=1, lib=oracle)
            s = T.ALSolver(q).solve()
            for k in keys:
                stats[k].append(s.stats[k][0])
            X.append(T.states(q)[0]); U.append(T.controls(q)[0])
        _linear[B, seed] = SimpleNamespace(B=B, stats={k: np.array(v) for k, v in stats.items()}, X=np.array(X), U=np.array(U)), models, bv
    return _linear[B, seed]
