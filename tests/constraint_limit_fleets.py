"""Fleets for per-trajectory constraint limits (to_set_constraint_limits_batch; tests/test_constraint_limits_oracle.py vets them on the CPU,
tests/test_gpu_constraint_limits.py holds the HIP library to them).  The reference is B single-trajectory ORACLE problems, problem b built
with trajectory b's own limit in its descriptor and — through ``batch=1, b_offset=b`` — its own start state (the scheme of
tests/model_params_fleet.py).  The oracle knows nothing about per-trajectory limits and is not changed.  Every draw comes from a seeded
generator; a reference is computed once per session and shared, and nothing in it is modified afterwards.

  cartpole / cartpole_split   Cartpole, |u| <= u_b on knots 1 .. N-1 and the goal at N (N = 101, tf = 5); u_b ~ U(2.7, 4.5) — `split`: u_max and
                              -u_min drawn separately.  (A lower edge of 2.4 leaves some Cartpoles at their iteration caps: stay at 2.7 or above.)
  dint                        2-D double integrator, N = 51, tf = 5, goal [1, 2, 0, 0] at N; ONE BoundConstraint on knots 1 .. N-1 with state and
                              control rows: x1 >= -0.5 (shared), x4 <= v_b ~ U(0.55, 0.9), u <= U(0.8, 1.6)^2, u >= -U(0.8, 1.6)^2 drawn
                              separately; x0[:2] ~ U(-0.2, 0.2).  Rows [x4 max, u1 max, u2 max, x1 min, u1 min, u2 min]: no fast layout.
  quadrotor                   C5 constraint set (goal on position + velocities, second-order cone on the controls), N = 61, tf = 3;
                              |u| <= a_b ~ U(4.5, 7.5); ALTRO with n_steps = C5_PN_STEPS.
"""
from types import SimpleNamespace

import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

OK = T.capi.SOLVE_SUCCEEDED
AL_KW = dict(constraint_tolerance=1e-4)
STAT_KEYS = ("iterations", "iterations_outer", "iterations_pn", "status", "cost", "c_max")
DINT_XF = np.array([1.0, 2.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------ draws
def cartpole_limits(B, split=False, seed=31, lo=2.7, hi=4.5):
    """-> (u_max [B], u_min [B])"""
    rng = np.random.default_rng(seed)
    up = rng.uniform(lo, hi, B)
    dn = rng.uniform(lo, hi, B) if split else up
    return up, -dn


def dint_limits(B, seed=32):
    """-> (v [B], u_max [B, 2], u_min [B, 2], x0 [B, 4])"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.55, 0.9, B)
    up = rng.uniform(0.8, 1.6, (B, 2))
    dn = rng.uniform(0.8, 1.6, (B, 2))
    x0 = np.zeros((B, 4))
    x0[:, :2] = rng.uniform(-0.2, 0.2, (B, 2))
    return v, up, -dn, x0


def quadrotor_limits(B, seed=37):
    return np.random.default_rng(seed).uniform(4.5, 7.5, B)


# ------------------------------------------------------------------------------------------------ problems
def cartpole_problem(lib, batch, b_offset=0, u_max=3.0, u_min=-3.0, model=None, N=101, tf=5.0):
    """configs.cartpole_problem(constrained=True) with a bound that need not be symmetric (for a symmetric one it IS that problem)."""
    if u_max == -u_min:
        return configs.cartpole_problem(batch=batch, b_offset=b_offset, N=N, tf=tf, constrained=True, u_bnd=u_max, lib=lib, model=model)
    p0 = configs.cartpole_problem(batch=1, N=N, tf=tf, constrained=True, lib=lib, model=model)
    n, m = p0.n, p0.m
    cons = T.ConstraintList(n, m, N)
    T.add_constraint(cons, T.BoundConstraint(n, m, u_min=u_min, u_max=u_max), range(1, N))
    T.add_constraint(cons, T.GoalConstraint(p0.xf), N)
    p = T.Problem(p0.model, p0.obj, np.zeros(n), tf, xf=p0.xf, constraints=cons, batch=batch, lib=lib)
    p.set_initial_state(configs.cartpole_x0(batch, b_offset))
    T.initial_controls(p, np.full(m, 0.01))
    return p


def dint_problem(lib, batch, x0, v=0.7, u_max=(1.2, 1.2), u_min=(-1.2, -1.2), N=51, tf=5.0):
    n, m = 4, 2
    obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 100 * np.ones(n), DINT_XF, N)
    cons = T.ConstraintList(n, m, N)
    T.add_constraint(cons, T.BoundConstraint(n, m, x_max=[np.inf, np.inf, np.inf, v], x_min=[-0.5, -np.inf, -np.inf, -np.inf],
                                             u_max=list(u_max), u_min=list(u_min)), (1, N - 1))
    T.add_constraint(cons, T.GoalConstraint(DINT_XF), N)
    p = T.Problem(T.DoubleIntegrator(1.0, 2), obj, np.zeros(n), tf, xf=DINT_XF, constraints=cons, batch=batch, lib=lib)
    p.set_initial_state(np.asarray(x0, dtype=np.float64).reshape(batch, n))
    return p


def quadrotor_problem(lib, batch, b_offset=0, a=6.0, model=None, N=61, tf=3.0):
    return configs.quadrotor_problem(batch=batch, b_offset=b_offset, N=N, tf=tf, constrained=True, goal_inds=configs.C5_GOAL_INDS,
                                     u_norm_max=a, lib=lib, model=model)


# ------------------------------------------------------------------------------------------------ fleets
class Spec:
    """One fleet: ``single(lib, b)`` — trajectory b's own problem, its limit in the descriptor; ``shared(lib, batch)`` — the batch with the
    nominal limit for everybody; ``set_limits(p)`` — the per-trajectory limits onto such a batch; ``margins(X, U)`` -> (by how much each
    trajectory leaves ITS limits, how close its control comes to one of them); ``con_id``: the flagged constraint; ``solvers``: name ->
    (solver class, keywords)."""

    def __init__(self, name, B):
        self.name, self.B, self.con_id = name, B, 0
        self.solvers = {"al": (T.ALSolver, AL_KW), "altro": (T.ALTROSolver, {})}
        if name.startswith("cartpole"):
            self.u_max, self.u_min = cartpole_limits(B, split=name == "cartpole_split", seed=31 if B <= 70 else 40)
            self.limits = np.stack([self.u_max, self.u_min], axis=1)               # rows [u max, u min]
        elif name == "dint":
            self.v, self.u_max, self.u_min, self.x0 = dint_limits(B)
            self.limits = np.concatenate([self.v[:, None], self.u_max, np.full((B, 1), -0.5), self.u_min], axis=1)
        elif name == "quadrotor":
            self.a = quadrotor_limits(B)
            self.limits = self.a[:, None]
            self.solvers["altro"] = (T.ALTROSolver, dict(n_steps=configs.C5_PN_STEPS))
        else:
            raise ValueError(name)

    def single(self, lib, b, **kw):
        if self.name.startswith("cartpole"):
            return cartpole_problem(lib, 1, b_offset=b, u_max=self.u_max[b], u_min=self.u_min[b], **kw)
        if self.name == "dint":
            return dint_problem(lib, 1, self.x0[b], v=self.v[b], u_max=self.u_max[b], u_min=self.u_min[b])
        return quadrotor_problem(lib, 1, b_offset=b, a=self.a[b], **kw)

    def shared(self, lib, **kw):
        if self.name.startswith("cartpole"):
            return cartpole_problem(lib, self.B, **kw)
        if self.name == "dint":
            return dint_problem(lib, self.B, self.x0)
        return quadrotor_problem(lib, self.B, **kw)

    def set_limits(self, p):
        if self.name.startswith("cartpole"):
            T.set_bounds_batch(p, 0, u_max=self.u_max[:, None], u_min=self.u_min[:, None])
        elif self.name == "dint":
            x_max = np.full((self.B, 4), np.inf); x_max[:, 3] = self.v
            T.set_bounds_batch(p, 0, x_max=x_max, u_max=self.u_max, u_min=self.u_min)
        else:
            T.set_constraint_limits_batch(p, 0, self.limits)

    def batch(self, lib, **kw):
        p = self.shared(lib, **kw)
        self.set_limits(p)
        return p

    def margins(self, X, U):
        if self.name.startswith("cartpole"):
            u = U[:, :, 0]
            out = np.maximum(u - self.u_max[:, None], self.u_min[:, None] - u).max(axis=1)
            return out, -out
        if self.name == "dint":
            gu = np.maximum(U - self.u_max[:, None, :], self.u_min[:, None, :] - U).max(axis=(1, 2))
            gx = np.maximum(X[:, :-1, 3] - self.v[:, None], -0.5 - X[:, :-1, 0]).max(axis=1)
            return np.maximum(gu, gx), -gu
        out = np.linalg.norm(U, axis=2).max(axis=1) - self.a
        return out, -out


def phases(p, con_id):
    """Everything the phase comparison looks at, after a rollout and two dual updates."""
    T.rollout(p); I.dual_update(p); I.dual_update(p)
    r = SimpleNamespace(c=T.evaluate_constraints(p, con_id), jac=T.constraint_jacobians(p, con_id), viol=T.max_violation(p), al=I.al_cost(p))
    I.expand(p); I.backwardpass(p)
    g = I.gains(p)
    r.K, r.d = g["K"], g["d"]
    r.ls, r.J = I.forwardpass(p)
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


def reference_phases(name, B, oracle):
    key = ("phases", name, B)
    if key not in _cache:
        s = spec(name, B)
        _cache[key] = _stack([phases(s.single(oracle, b), s.con_id) for b in range(B)])
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


def reference_solve(name, B, solver, oracle):
    """The B singles solved with ``solver`` ("al" / "altro"), stacked: .stats, .X, .U, .total_iterations."""
    key = ("solve", name, B, solver)
    if key not in _cache:
        s = spec(name, B)
        Solver, kw = s.solvers[solver]
        _cache[key] = solve_singles([s.single(oracle, b) for b in range(B)], Solver, kw)
    return _cache[key]


def nudged(p, eps):
    """The problem with its control guess moved by eps (1 + |u|) — far below anything a tolerance of the tests sees."""
    U = T.controls(p)
    T.initial_controls(p, U + eps * (1.0 + np.abs(U)))
    return p


def nudged_solve(name, B, solver, oracle, eps):
    """The B singles solved from the nudged control guess (see nudged_iterations)."""
    key = ("nudged", name, B, solver, eps)
    if key not in _cache:
        s = spec(name, B)
        Solver, kw = s.solvers[solver]
        _cache[key] = solve_singles([nudged(s.single(oracle, b), eps) for b in range(B)], Solver, kw)
    return _cache[key]


def nudged_iterations(name, B, solver, oracle, eps):
    """Iteration counts of the B singles started from a control guess moved by eps: a trajectory whose count changes under a 1e-12 nudge sits
    on a decision boundary of the solver (a line search or a convergence test within rounding of a tie) — two correct implementations that
    round differently may disagree on its integers, so such a trajectory cannot be in a fleet that is compared bit for bit."""
    return nudged_solve(name, B, solver, oracle, eps).stats["iterations"]


def shared_solve(name, B, solver, oracle):
    """The same fleet with the nominal limit for every trajectory (one oracle batch)."""
    key = ("shared", name, B, solver)
    if key not in _cache:
        s = spec(name, B)
        Solver, kw = s.solvers[solver]
        p = s.shared(oracle)
        st = Solver(p, **kw).solve().stats
        _cache[key] = SimpleNamespace(stats={k: st[k].copy() for k in STAT_KEYS}, X=T.states(p), U=T.controls(p))
    return _cache[key]


def assert_solve_parity_fleet(sh, ph, ref, po, rtol):
    """tests/test_gpu_parity.py assert_solve_parity with the stacked singles in the oracle batch's place: ``po`` is an oracle batch of the
    fleet's shape that is handed the singles' trajectories, ``ref`` answers for the solver (stats, total_iterations)."""
    from test_gpu_parity import assert_solve_parity
    T.initial_states(po, ref.X); T.initial_controls(po, ref.U)
    assert_solve_parity(sh, ref, ph, po, rtol=rtol)


# ------------------------------------------------------------------------------------------------ combination: plants + goals + limits
def combo(B=70):
    """Cartpole with plants, goals (with the GoalConstraint's target) and limits all per trajectory: -> (models, Xf, u_max, u_min)."""
    import model_params_fleet as F
    models = F.draw_models("cartpole_con", B, 50, spread=0.1)
    Xf = F.cartpole_goal_fleet(B, con=True)
    up, dn = cartpole_limits(B, seed=150, lo=3.0, hi=4.5)
    return models, Xf, up, dn


def combo_single(lib, b):
    models, Xf, up, dn = _cache.setdefault("combo", combo())
    p = cartpole_problem(lib, 1, b_offset=b, u_max=up[b], u_min=dn[b], model=models[b])
    T.set_goal_state(p, Xf[b])
    return p


def combo_reference(oracle, solver="altro", B=70):
    key = ("combo", solver)
    if key not in _cache:
        Solver, kw = {"al": (T.ALSolver, AL_KW), "altro": (T.ALTROSolver, {})}[solver]
        _cache[key] = solve_singles([combo_single(oracle, b) for b in range(B)], Solver, kw)
    return _cache[key]
