"""Reference for per-trajectory model parameters (tests/test_gpu_model_params_batch.py): B single-trajectory ORACLE problems, problem b
built with its own model and — through ``batch=1, b_offset=b`` — with trajectory b's own start state (the scheme of
tests/test_goal_batch.py).  The oracle itself knows nothing about per-trajectory parameters and is not changed.  A fleet is computed once
per configuration and shared by the tests that need it (``fleet``); nothing in it is modified afterwards."""
import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

SPREAD = 0.2  # parameters within +-20 % of the configuration's values


def draw_models(kind, B, seed, spread=SPREAD):
    """B models of the problem's class, parameters drawn uniformly within +-spread of the nominal ones by a seeded generator; model 0 keeps
    the nominal (shared) values.  Cartpole: cart mass, pole mass, pole length; Quadrotor: mass, the three inertias, the torque constant
    km; double integrator: the mass.  (Gravity, the motor geometry and the entries that select dimensions stay the problem's.)"""
    rng = np.random.default_rng(seed)
    f = lambda k: 1.0 + spread * rng.uniform(-1.0, 1.0, (B, k))
    if kind.startswith("cartpole"):
        s = f(3)
        models = [T.Cartpole(mc=1.0 * a, mp=0.2 * b, l=0.5 * c) for a, b, c in s]
        models[0] = T.Cartpole()
    elif kind == "quadrotor":
        s = f(5)
        models = [T.Quadrotor(mass=0.5 * a, J=(0.0023 * b, 0.0023 * c, 0.004 * d), km=0.0245 * e) for a, b, c, d, e in s]
        models[0] = T.Quadrotor()
    elif kind == "dint":
        s = f(1)
        models = [T.DoubleIntegrator(1.0 * a, 2) for (a,) in s]
        models[0] = T.DoubleIntegrator(1.0, 2)
    else:
        raise ValueError(kind)
    return models


def params_of(models):
    pp = np.zeros((len(models), 16))
    for b, mod in enumerate(models):
        q = mod.params()
        pp[b, : len(q)] = q
    return pp


def build(kind, lib, batch, b_offset=0, model=None, N=None, tf=None, x0=None):
    """The problem of a configuration on ``lib``; ``model``: the model it is built on (default: the nominal one); ``x0``: one start state for
    every trajectory instead of the configuration's per-trajectory ones."""
    if kind == "cartpole":
        p = configs.cartpole_problem(batch=batch, N=N or 31, tf=tf or 1.5, b_offset=b_offset, lib=lib, model=model)
    elif kind == "cartpole_con":
        p = configs.cartpole_problem(batch=batch, N=N or 51, tf=tf or 2.5, b_offset=b_offset, constrained=True, u_bnd=10.0, lib=lib, model=model)
    elif kind == "quadrotor":
        p = configs.quadrotor_problem(batch=batch, N=N or 41, tf=tf or 1.0, b_offset=b_offset, lib=lib, model=model)
    elif kind == "dint":
        n, m, Nn = 4, 2, N or 31
        mdl = model if model is not None else T.DoubleIntegrator(1.0, 2)
        xf = np.array([1.0, 2.0, 0.0, 0.0])
        obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 100 * np.ones(n), xf, Nn)
        cons = T.ConstraintList(n, m, Nn)
        T.add_constraint(cons, T.BoundConstraint(n, m, u_max=1.5, u_min=-1.5), (1, Nn - 1))
        p = T.Problem(mdl, obj, np.zeros(n), tf or 3.0, xf=xf, constraints=cons, batch=batch, lib=lib)
        b = np.arange(b_offset, b_offset + batch, dtype=np.uint64)
        X0 = np.zeros((batch, n))
        X0[:, 0] = configs.splitmix64_uniform(7, 2 * b) - 0.5
        X0[:, 1] = configs.splitmix64_uniform(7, 2 * b + np.uint64(1)) - 0.5
        p.set_initial_state(X0)
    else:
        raise ValueError(kind)
    if x0 is not None:
        p.set_initial_state(np.tile(np.asarray(x0, dtype=np.float64), (batch, 1)))
    return p


SOLVERS = {"ilqr": T.iLQRSolver, "al": T.ALSolver, "altro": T.ALTROSolver}


class Fleet:
    """Results of B single-trajectory oracle problems, stacked along the batch axis."""

    def __init__(self, kind, oracle, models, solver=None, phases=False, x0=None, sel=None, **kw):
        """``sel``: the trajectories to run (default: all of them), e.g. a sample of a large batch."""
        sel = range(len(models)) if sel is None else sel
        self.B = len(sel)
        keys = ("iterations", "iterations_outer", "iterations_pn", "status", "cost", "c_max")
        self.stats = {k: [] for k in keys}
        rows = {k: [] for k in ("X", "U", "Xr", "J", "F", "A", "Bm", "K", "d", "ls", "Jn", "defect")}
        for b in sel:
            p = build(kind, oracle, 1, b_offset=int(b), model=models[b], x0=x0, **kw)
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
                s = SOLVERS[solver](p).solve()
                for k in keys:
                    self.stats[k].append(s.stats[k][0])
                rows["X"].append(T.states(p)[0]); rows["U"].append(T.controls(p)[0])
        self.stats = {k: np.array(v) for k, v in self.stats.items() if v}
        for k, v in rows.items():
            if v:
                setattr(self, k, np.array(v))
        if solver:
            self.total_iterations = int(self.stats["iterations"].sum())


_cache = {}


def fleet(kind, oracle, B, seed, solver=None, phases=False, x0=None, sel=None, **kw):
    """The fleet of a configuration, computed once per session."""
    key = (kind, B, seed, solver, phases, None if x0 is None else tuple(x0), None if sel is None else tuple(sel), tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = Fleet(kind, oracle, draw_models(kind, B, seed), solver=solver, phases=phases, x0=x0, sel=sel, **kw)
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
