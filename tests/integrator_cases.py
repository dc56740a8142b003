"""RK3 and Euler on every kernel path that integrates: rows (a batch, a solver, one of the two non-default schemes) and a numpy
longdouble restatement of the three schemes that goes through no solver code.

A model with ``pin_rk4`` (the double integrators, the Cartpole, the hybrid double integrator, the model vector, InfeasibleModel) runs a
second set of kernel instances for an RK3 or Euler handle (``FIXED_INTEG = -1``); for the Quadrotors the scheme is a run-time branch
of ``rk_step``.  Either way a non-RK4 handle runs code that the RK4 rows of the other test files never reach.

Shared by tests/test_integrator_cases_oracle.py (which vets every row on the CPU oracle alone and holds the oracle's step to the
restatement) and tests/test_gpu_integrators.py (which runs the rows on every kernel path).  No GPU is needed to import this module.

The rows are option_cases.Row objects without overrides over failure_cases.Case objects, so that ``build(lib, ulp, **opts)``,
``solve``, ``first_pass``, option_cases.stability and test_gpu_options.assert_row_solve take them as they are.

The host mirror passes ``integration`` through for all three phase-only models (InfeasibleProblem copies it from the problem it
lifts; a model vector's Problem hands it to the library like any other): nothing is refused, and the rows run with RK3.

The restatement (``step`` / ``rollout``) is written from the formulas: stage slopes multiplied by h;
RK4: x + (k1 + 2 k2 + 2 k3 + k4) / 6 with stages at x + k1/2, x + k2/2, x + k3;
RK3: x + (k1 + 4 k2 + k3) / 6 with stages at x + k1/2 and x - k1 + 2 k2;  Euler: x + h f —
over the Cartpole of docs/src/model.md (qdd = -H \\ (C qd + G - B u)) and the D-dimensional double integrator (xdot = [v, u / mass])."""
import math

import numpy as np

import trajopt_amd as T
from trajectoryoptimization_jl_amd import configs
import failure_cases as F
import option_cases as O

L = np.longdouble
SCHEMES = {"rk3": T.RK3, "euler": T.Euler}
TAGS = {T.RK4: "rk4", T.RK3: "rk3", T.Euler: "euler"}
TRIG_SMALL_MAX = 0.75      # models.h: beyond it a lane of trig_stage takes the full sin / cos evaluation


# ------------------------------------------------------------------------------------------------------------------ the restatement
def cartpole_f(x, u, mc=1.0, mp=0.2, l=0.5, g=9.81):
    """xdot of the Cartpole, x = (p, theta, pdot, thetadot) [..., 4], u [..., 1]: qdd = -H \\ (C qd + G - B u) with
    H = [mc + mp, mp l c; mp l c, mp l^2], C = [0, -mp thetadot l s; 0, 0], G = [0, mp g l s], B = [1, 0]."""
    x, u = np.asarray(x, L), np.asarray(u, L)
    mc, mp, l, g = L(mc), L(mp), L(l), L(g)
    th, pd, thd = x[..., 1], x[..., 2], x[..., 3]
    s, c = np.sin(th), np.cos(th)
    h11, h12, h22 = mc + mp, mp * l * c, mp * l * l
    r1 = -(-mp * thd * l * s * thd - u[..., 0])       # -(C qd + G - B u)
    r2 = -(mp * g * l * s)
    det = h11 * h22 - h12 * h12
    return np.stack([pd, thd, (h22 * r1 - h12 * r2) / det, (h11 * r2 - h12 * r1) / det], axis=-1)


def double_integrator_f(mass, D):
    def f(x, u):
        x, u = np.asarray(x, L), np.asarray(u, L)
        return np.concatenate([x[..., D:], u / L(mass)], axis=-1)
    return f


def stages(f, scheme, x, u, h):
    """-> (the stage points after the first, the slopes k_i = h f(stage i)) of one step."""
    x, h = np.asarray(x, L), L(h)
    k1 = h * f(x, u)
    if scheme == T.Euler:
        return [], [k1]
    x2 = x + k1 / 2
    k2 = h * f(x2, u)
    if scheme == T.RK3:
        x3 = x - k1 + 2 * k2
        return [x2, x3], [k1, k2, h * f(x3, u)]
    assert scheme == T.RK4
    x3 = x + k2 / 2
    k3 = h * f(x3, u)
    x4 = x + k3
    return [x2, x3, x4], [k1, k2, k3, h * f(x4, u)]


def step(f, scheme, x, u, h):
    """One step of the scheme in extended precision, x [..., n], u [..., m] -> [..., n] (longdouble)."""
    _, k = stages(f, scheme, x, u, h)
    x = np.asarray(x, L)
    if scheme == T.Euler:
        return x + k[0]
    if scheme == T.RK3:
        return x + (k[0] + 4 * k[1] + k[2]) / 6
    return x + (k[0] + 2 * k[1] + 2 * k[2] + k[3]) / 6


def rollout(f, scheme, x0, U, h):
    """x0 [B, n], U [B, N-1, m], h a step size or [N-1] of them -> X [B, N, n] (longdouble)."""
    U = np.asarray(U, L)
    hs = np.broadcast_to(np.asarray(h, L), (U.shape[1],))
    X = [np.asarray(x0, L)]
    for k in range(U.shape[1]):
        X.append(step(f, scheme, X[-1], U[:, k], hs[k]))
    return np.stack(X, axis=1)


def cartpole_stage_deltas(scheme, x, u, h):
    """The angle increments theta_stage - theta of the later stages of one Cartpole step, [..., stages - 1] (what trig_stage is
    handed as delta); empty for Euler."""
    pts, _ = stages(cartpole_f, scheme, x, u, h)
    x = np.asarray(x, L)
    return np.stack([p[..., 1] - x[..., 1] for p in pts], axis=-1) if pts else np.zeros(x.shape[:-1] + (0,), L)


def restatement_of(p):
    """-> the dynamics of the problem's model for ``rollout``, or None (the Quadrotors and the model vectors have none here)."""
    if isinstance(p.model, T.Cartpole):
        m = p.model
        return lambda x, u: cartpole_f(x, u, m.mc, m.mp, m.l, m.g)
    if isinstance(p.model, T.DoubleIntegrator):
        return double_integrator_f(p.model.mass, p.model.D)
    return None


# -------------------------------------------------------------------------------------------------------------------------- builders
def _config(fn, **fixed):
    """A builder over one of the configs.* problems, ``integration`` and the solver options passed through."""
    def make(integration, **base):
        def build(lib, extra):
            o = F._options(lib, base, extra)
            p = fn(lib=lib, options=o, integration=integration, **fixed)
            p.case_options = o
            return p
        return build
    return make


def _di2(integration, **base):
    return F._double_integrator(u_bnd=2.0, amp=4.0, integration=integration, **base)


def _di3(integration, B=70, N=21, tf=2.0, **base):
    """DoubleIntegrator(., 3), unconstrained: ne = 6, m = 3 — neither the scan kernel's nor the 8-lane cooperative shape.  With
    positive weights the problem is linear-quadratic and iLQR is done after one full step (two iterations, on the oracle); the
    negative control weight of failure_cases.di2_uniform makes Quu indefinite, the backward pass regularises (rho = 5.99 on the first
    pass) and the damped steps go on to the iteration cap of six."""
    def build(lib, extra):
        model = T.DoubleIntegrator(0.8, 3)
        n, m = model.dims()
        xf = np.array([1.0, -2.0, 0.5, 0.0, 0.0, 0.0])
        obj = T.LQRObjective(np.ones(n), np.array([0.1, -0.09, 0.05]), np.array([10.0, 20.0, 5.0, 10.0, 10.0, 10.0]), xf, N, checks=False)
        o = F._options(lib, base, extra)
        p = T.Problem(model, obj, np.zeros(n), tf, xf=xf, constraints=T.ConstraintList(n, m, N), batch=B, lib=lib, options=o,
                      integration=integration)
        p.case_options = o
        p.set_initial_state(np.linspace(-0.5, 0.5, B)[(17 * np.arange(B)) % B][:, None] * np.ones((B, n)))
        b, k, j = np.arange(B)[:, None, None], np.arange(N - 1)[None, :, None], np.arange(m)[None, None, :]
        T.initial_controls(p, 4.0 * F._spread(B)[:, None, None] * np.sin(0.3 * k + 0.1 * b + 1.3 * j))
        return p
    return build


def _mrp(integration, B=24, **base):
    def build(lib, extra):
        from test_gpu_parity import _mrp_quadrotor
        o = F._options(lib, base, extra)
        p = _mrp_quadrotor(lib, False, B, integration=integration, options=o)
        p.case_options = o
        return p
    return build


_cartpole = _config(configs.cartpole_problem, batch=70, N=41, tf=2.0)
_cartpole_con = _config(configs.cartpole_problem, batch=70, N=41, tf=2.0, constrained=True)
_quadrotor = _config(configs.quadrotor_problem, batch=24, N=21, tf=1.0)
_quadrotor_con = _config(configs.quadrotor_problem, batch=24, N=21, tf=1.0, constrained=True)
_cartpole_polish = _config(configs.cartpole_problem, batch=70, N=41, tf=2.0, constrained=True, u_bnd=10.0)
_quadrotor_polish = _config(configs.quadrotor_problem, batch=24, N=21, tf=2.0, constrained=True, goal_inds=configs.C5_GOAL_INDS)

# base name -> (builder factory, solver, creation options, small model, schemes)
_BASES = {
    "cartpole_ilqr": (_cartpole, "ilqr", dict(iterations=25), True, ("rk3", "euler")),
    "cartpole_al": (_cartpole_con, "al", dict(iterations=20, iterations_outer=3), True, ("rk3", "euler")),
    "di2_al": (_di2, "al", dict(), True, ("rk3", "euler")),
    "di3_ilqr": (_di3, "ilqr", dict(iterations=6), True, ("rk3", "euler")),
    "quadrotor_ilqr": (_quadrotor, "ilqr", dict(iterations=8), False, ("rk3", "euler")),
    "quadrotor_al": (_quadrotor_con, "al", dict(iterations=5, iterations_outer=4), False, ("rk3", "euler")),
    "quadrotor_mrp_ilqr": (_mrp, "ilqr", dict(iterations=8), False, ("rk3",)),
    # the polish.  The AL rows above cannot serve: with |u| <= 3 the Cartpole does not reach the goal within 2 s (its AL stage ends
    # MAX_ITERATIONS_OUTER / MAXIMUM_COST with a violation of 1 .. 2 at any iteration cap, and with RK3 at horizons of 3 s and 4 s too), and the
    # Quadrotor's 13-state goal pins the quaternion, which no Runge-Kutta scheme keeps on the unit sphere, within 1 s — to_altro_solve
    # skips the polish for every trajectory.  The ALTRO rows therefore take the bound of smoke() (|u| <= 10) on the Cartpole and the
    # goal on position and velocities (configs.C5_GOAL_INDS) over 2 s on the Quadrotor, default options: on the oracle every trajectory of
    # them ends its AL stage SOLVE_SUCCEEDED and is projected once or twice (test_integrator_cases_oracle.py asserts the share, POLISHED).
    "cartpole_altro": (_cartpole_polish, "altro", dict(), True, ("rk3", "euler")),
    "quadrotor_altro": (_quadrotor_polish, "altro", dict(), False, ("rk3",)),
    # the Quadrotor with Euler: at h = 0.1 .. 0.025 the AL stage of the same problem runs into its limits for most of the batch (on the
    # oracle: 5 of 24 trajectories polished after 7 s at N = 21, 12 of 24 after 11 s at N = 41; statuses 3, 4, 5, 11 next to 2), far too
    # slow a row to vet nine times.  The Euler row keeps the capped AL problem and asserts what to_altro_solve does with it: no
    # trajectory is handed to the polish.  The Euler branch of the polish's model_step runs on the Cartpole row.
    "quadrotor_altro_unpolished": (_quadrotor_con, "altro", dict(iterations=5, iterations_outer=4), False, ("euler",)),
    "di2_altro": (_di2, "altro", dict(), True, ("rk3", "euler")),
}
# base -> the least share of the batch that the polish must project at least once (0: none may be)
POLISHED = {"cartpole_altro": 0.75, "quadrotor_altro": 0.75, "di2_altro": 0.5, "quadrotor_altro_unpolished": 0.0}
ROWS, RK4_ROWS, BASE_OF, SCHEME_OF = {}, {}, {}, {}


def _row(base, tag, integration):
    make, solver, opts, small, _ = _BASES[base]
    name = f"{base}_{tag}"
    return O.Row(name, F.Case(name, make(integration, **opts), solver, expect=[], statuses=[], small=small), {})


for _base, _spec in _BASES.items():
    RK4_ROWS[_base] = _row(_base, "rk4", T.RK4)
    for _tag in _spec[4]:
        _r = _row(_base, _tag, SCHEMES[_tag])
        ROWS[_r.name], BASE_OF[_r.name], SCHEME_OF[_r.name] = _r, _base, SCHEMES[_tag]

ALTRO = [n for n, r in ROWS.items() if r.solver == "altro"]
SOLVE = [n for n, r in ROWS.items() if r.solver != "altro"]
# RK3 of xdot = [v, u / mass] under a control held over the step is exact, like RK4 (the solution is a quadratic in t, both schemes
# reproduce polynomials of degree <= 3): on the double integrators RK3 and RK4 compute the same step up to rounding, and the row
# cannot differ from its RK4 run.  These rows still run the RK3 instances of every kernel; Euler does differ.
SAME_AS_RK4 = [n for n in ROWS if BASE_OF[n].startswith("di") and SCHEME_OF[n] == T.RK3]


# ----------------------------------------------------------------------------------------------------------------- phase-only rows
def _infeasible_cartpole(lib, integration):
    from test_infeasible import cartpole_infeasible
    return cartpole_infeasible(lib, integration=integration)[0]


def _live_controls(p):
    """Random controls on the live entries of every step of a model vector (with zero controls Euler and RK4 move a double
    integrator alike); the padding stays zero."""
    rng = np.random.default_rng(2)
    U = np.zeros((p.B, p.N - 1, p.m))
    for k, mk in enumerate(p.nu[:-1]):
        U[:, k, :mk] = rng.uniform(-1, 1, (p.B, mk))
    T.initial_controls(p, U)
    return p


def _hybrid(lib, integration):
    from test_hybrid_dims import hybrid_problem
    return _live_controls(hybrid_problem(lib, batch=5, integration=integration)[0])


def _vector_cartpole_mix(lib, integration):
    import test_model_vector as MV
    return _live_controls(MV.build(MV.cartpole_mix(), lib, batch=5, integration=integration)[0])


# (rollout / Jacobians / expansion / gains, no solve)
PHASE_ONLY = {"infeasible_cartpole": _infeasible_cartpole, "hybrid": _hybrid, "vector_cartpole_mix": _vector_cartpole_mix}
# RK3 each; the hybrid double integrator with Euler as well: RK3 and RK4 agree to rounding on its linear steps, so only Euler can tell
# whether the handle runs the scheme it was given
PHASE_ONLY_CASES = [("infeasible_cartpole", T.RK3), ("hybrid", T.RK3), ("hybrid", T.Euler), ("vector_cartpole_mix", T.RK3)]


# --------------------------------------------------------------------------------------------------------- the angle-addition batch
THRESHOLD_B, THRESHOLD_N, THRESHOLD_DT = 192, 5, 0.05
NEAR = 1e-3


def largest_delta(scheme, thd, x_rest, u, h=THRESHOLD_DT):
    """|delta| of the scheme's largest later stage on the first step (RK4: the fourth stage, delta = k3; RK3: the third,
    2 k2 - k1) from the state (x_rest with thetadot = thd)."""
    x = np.array(x_rest, L)
    x[..., 3] = thd
    return np.abs(cartpole_stage_deltas(scheme, x, u, h)[..., -1])


def _solve_thd(scheme, target, x_rest, u, sign):
    """thetadot of the given sign whose largest first-step delta is ``target`` (bisection on the restatement; the delta grows with
    |thetadot| over the bracket)."""
    lo, hi = L(5.0), L(40.0)
    for _ in range(80):
        mid = (lo + hi) / 2
        if largest_delta(scheme, sign * mid, x_rest, u) < target:
            lo = mid
        else:
            hi = mid
    return float(sign * hi)


def threshold_batch(scheme):
    """-> (x0 [192, 4], U [192, 4, 1]) float64: three waves of the rollout's map.  Wave 0: |thetadot| <= 8, every stage delta of every
    step far below 0.75; wave 2: |thetadot| in [22, 32], the largest stage's delta above 0.75 at every step; wave 1: lanes alternate
    between |thetadot| ~ 9 and ~ 21, except eight lanes whose largest first-step delta sits within 1e-3 of the threshold, four on each
    side.  Euler has no later stage: it runs the RK4 batch."""
    s = T.RK4 if scheme == T.Euler else scheme
    B = THRESHOLD_B
    rng = np.random.default_rng(41)
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(-0.5, 0.5, B)
    x0[:, 1] = rng.uniform(-math.pi, math.pi, B)
    x0[:, 2] = rng.uniform(-1.0, 1.0, B)
    U = rng.uniform(-2.0, 2.0, (B, THRESHOLD_N - 1, 1))
    sign = np.where(np.arange(B) % 4 < 2, 1.0, -1.0)
    lane = np.arange(64)
    x0[:64, 3] = sign[:64] * rng.uniform(0.0, 8.0, 64)
    x0[128:, 3] = sign[128:] * rng.uniform(22.0, 32.0, 64)
    x0[64:128, 3] = sign[64:128] * np.where(lane % 2 == 0, rng.uniform(8.0, 10.0, 64), rng.uniform(20.0, 22.0, 64))
    # eight lanes of wave 1 at the threshold: even lanes just below, odd lanes just above
    for i, ln in enumerate((10, 11, 26, 27, 40, 41, 58, 59)):
        b = 64 + ln
        off = (0.2 + 0.2 * (i // 2)) * NEAR               # 2e-4 .. 8e-4 from the threshold
        target = TRIG_SMALL_MAX - off if ln % 2 == 0 else TRIG_SMALL_MAX + off
        x0[b, 3] = _solve_thd(s, L(target), x0[b], U[b, 0], sign[b])
    return x0, U


def threshold_deltas(scheme, x0, U):
    """-> [B, N-1] the largest later stage's |delta| at every step of the restated rollout of the batch."""
    s = T.RK4 if scheme == T.Euler else scheme
    X = rollout(cartpole_f, s, x0, U, THRESHOLD_DT)
    return np.stack([np.abs(cartpole_stage_deltas(s, X[:, k], np.asarray(U, L)[:, k], THRESHOLD_DT)).max(axis=-1)
                     for k in range(U.shape[1])], axis=1)


def threshold_problem(lib, scheme, x0, U):
    p = configs.cartpole_problem(batch=THRESHOLD_B, N=THRESHOLD_N, tf=THRESHOLD_DT * (THRESHOLD_N - 1), integration=scheme, lib=lib)
    p.set_initial_state(x0)
    T.initial_controls(p, U)
    return p
