"""Fleets for per-trajectory attitude references (to_set_cost_attitude_batch / to_set_tracking_attitude; tests/test_attitude_fleets_oracle.py
vets them on the CPU, tests/test_gpu_cost_attitude.py holds the HIP library to them).  The reference is B single-trajectory ORACLE problems,
problem b built with trajectory b's own q_ref in its DiagonalQuatCost descriptors and — through ``batch=1, b_offset=b`` — its own start
state (the scheme of tests/cost_weight_fleets.py).  The oracle knows nothing about per-trajectory attitudes and is not changed.  Every draw
comes from a seeded generator; a reference is computed once per session and shared, and nothing in it is modified afterwards.

  goal      Quadrotor, N = 31, tf = 1, the QuatLQRCost pair of cost_weight_fleets._quadrotor_nominal (w = 1; Q is zero on the quaternion
            entries, so the attitude goal lives in w min(1 +- q_ref'q) alone).  Per trajectory: goal position = nominal + U(-0.5, 0.5)^3, goal
            attitude = a rotation by U(45, 180) degrees about the normalised axis [0.2 U(-1, 1), 0.2 U(-1, 1), 1]: four non-zero
            components that differ by trajectory.  A single carries the NOMINAL constant c — what ``set_goal_state`` leaves on the batch.
            Variants ``free`` and ``bound`` (0 <= u <= 3 on knots 1 .. N-1).  B = 24 (solves), B = 70 (phases: two tiles, the second partial).
  tracking  Quadrotor, N = 21, tf = 1, Nref = 30, one DiagonalQuatCost per knot: Q = diag(10, 10, 10, 0, 0, 0, 0, 1, .., 1), ten times that on
            the terminal knot, R = 1e-2, w = 1.  Each trajectory follows its own helix through its start position (radius U(0.5, 1.5), rate
            +-U(0.5, 2) rad/s, phase U(0, 2 pi), climb U(-0.3, 0.3) m/s, consistent velocities, yaw along the heading, hover u_ref); window
            starts uniform in 1 .. 20 under HOLD, so the later windows run past the end of the reference.
"""
import math
from types import SimpleNamespace

import numpy as np

import trajopt_amd as T
from trajectoryoptimization_jl_amd import configs
import cost_weight_fleets as F

OK = F.OK
SOLVERS, STAT_KEYS, variant_of, relerr, solve_singles, ulp_moved = F.SOLVERS, F.STAT_KEYS, F.variant_of, F.relerr, F.solve_singles, F.ulp_moved
INTEGERS = ("iterations", "iterations_outer", "iterations_pn", "status")
U_MAX = 3.0
SEEDS = {"goal": 411, "tracking": 412}
# X / U tolerance of the solves per (fleet, B, solver) where the default — 1e-6, 1e-5 for AL — is below the oracle's own +-1-ulp spread with
# the margin of tests/test_oracle_sensitivity.py (tests/test_attitude_fleets_oracle.py measures it; empty: every default holds)
SOLVE_RTOL = {}
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])


def solve_rtol(name, B, solver):
    return SOLVE_RTOL.get((name, B, solver), 1e-5 if solver == "al" else 1e-6)


def _constraints(variant, N):
    cons = T.ConstraintList(13, 4, N)
    if variant == "bound":
        T.add_constraint(cons, T.BoundConstraint(13, 4, u_min=0.0, u_max=U_MAX), range(1, N))
    elif variant != "free":
        raise ValueError(variant)
    return cons


class GoalFleet:
    """``single(lib, b, variant)``: trajectory b's own problem, its goal (position AND attitude) in the descriptors; ``shared(lib, variant)``:
    the batch on the nominal goal; ``batch(lib, variant)``: the per-trajectory goals onto such a batch through
    ``T.set_goal_state(p, Xf, attitude=True)`` (``attitude=False``: the positions alone, every member on the nominal attitude)."""
    name, N, tf = "goal", 31, 1.0

    def __init__(self, B):
        self.B = B
        rng = np.random.default_rng(SEEDS["goal"])
        self.Q0, self.R0, self.Qf0, self.xf, self.uf = F._quadrotor_nominal()
        Xf = np.tile(self.xf, (B, 1))
        Xf[:, :3] += rng.uniform(-0.5, 0.5, (B, 3))
        ang = np.radians(rng.uniform(45.0, 180.0, B))
        ax = np.c_[0.2 * rng.uniform(-1, 1, (B, 2)), np.ones(B)]
        ax /= np.linalg.norm(ax, axis=1)[:, None]
        Xf[:, 3] = np.cos(ang / 2)
        Xf[:, 4:7] = np.sin(ang / 2)[:, None] * ax
        self.Xf = Xf
        self.Xf.setflags(write=False)

    def _problem(self, lib, batch, b_offset, xf, q_ref, variant):
        """costs on the goal ``xf`` with attitude reference ``q_ref`` and the constants of the NOMINAL goal (no setter touches c)"""
        Q0, R0, Qf0, uf = self.Q0, self.R0, self.Qf0, self.uf
        c0 = 0.5 * self.xf @ (Q0 * self.xf) + 0.5 * uf @ (R0 * uf)
        cf0 = 0.5 * self.xf @ (Qf0 * self.xf) + 0.5 * uf @ (R0 * uf)
        stage = T.DiagonalQuatCost(Q0, R0, -Q0 * xf, -R0 * uf, c0, 1.0, q_ref)
        term = T.DiagonalQuatCost(Qf0, R0, -Qf0 * xf, -R0 * uf, cf0, 1.0, q_ref, terminal=True)
        p = T.Problem(T.Quadrotor(), T.Objective(stage, term, self.N), np.zeros(13), self.tf, xf=xf, constraints=_constraints(variant, self.N), batch=batch, lib=lib)
        p.set_initial_state(configs.quadrotor_x0(batch, b_offset))
        T.initial_controls(p, uf)
        return p

    def single(self, lib, b, variant="free", attitude=True):
        return self._problem(lib, 1, b, self.Xf[b], self.Xf[b, 3:7] if attitude else self.xf[3:7], variant)

    def shared(self, lib, variant="free", batch=None, b_offset=0):
        return self._problem(lib, self.B if batch is None else batch, b_offset, self.xf, self.xf[3:7], variant)

    def batch(self, lib, variant="free", attitude=True):
        p = self.shared(lib, variant)
        T.set_goal_state(p, np.array(self.Xf), constraint=False, attitude=attitude)
        return p


class TrackingFleet:
    """``problem(lib, rows, variant)``: the batch on its initial shared reference (a tracking objective: one DiagonalQuatCost per knot);
    ``single(lib, b, start, variant, attitude)``: trajectory b alone, every knot's cost built on ITS reference knot — linear terms and
    (``attitude``) q_ref —, held at the last knot past the end; ``Xref`` [B, Nref, 13], ``Uref`` [B, Nref, 4], ``start`` [B]."""
    name, N, tf, Nref = "tracking", 21, 1.0, 30
    Qd = np.array([10.0, 10, 10, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1])
    Rd = np.full(4, 1e-2)

    def __init__(self, B):
        self.B = B
        N, Nref = self.N, self.Nref
        rng = np.random.default_rng(SEEDS["tracking"])
        self.uf = T.Quadrotor().hover_control()
        self.x0 = configs.quadrotor_x0(B, 0)
        rad, om = rng.uniform(0.5, 1.5, B), rng.uniform(0.5, 2.0, B) * rng.choice([-1, 1], B)
        phi, climb = rng.uniform(0, 2 * np.pi, B), rng.uniform(-0.3, 0.3, B)
        t = np.arange(Nref) * (self.tf / (N - 1))
        Xref, Uref = np.zeros((B, Nref, 13)), np.tile(self.uf, (B, Nref, 1))
        for b in range(B):
            a = phi[b] + om[b] * t
            c = self.x0[b, :3] - rad[b] * np.array([math.cos(phi[b]), math.sin(phi[b]), 0.0])
            Xref[b, :, 0], Xref[b, :, 1], Xref[b, :, 2] = c[0] + rad[b] * np.cos(a), c[1] + rad[b] * np.sin(a), c[2] + climb[b] * t
            Xref[b, :, 7], Xref[b, :, 8], Xref[b, :, 9] = -rad[b] * om[b] * np.sin(a), rad[b] * om[b] * np.cos(a), climb[b]
            yaw = a + np.pi / 2 * np.sign(om[b])       # along the heading
            Xref[b, :, 3], Xref[b, :, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        self.Xref, self.Uref = Xref, Uref
        self.start = rng.integers(1, 21, B).astype(np.int32)     # HOLD: the windows of the later starts run past the end
        self.start2 = (1 + (self.start + 6 + np.arange(B) % 5) % 29).astype(np.int32)   # a second set of windows, 1 .. 29
        for a in (self.Xref, self.Uref, self.start, self.start2):
            a.setflags(write=False)

    def W(self, k):
        return self.Qd * (10.0 if k == self.N - 1 else 1.0)

    def _costs(self, x, u, q_ref):
        """x [N, 13], u [N, 4], q_ref [N, 4]: knot k's cost on (x[k], u[k]) with attitude reference q_ref[k]; c = 0"""
        N = self.N
        return [T.DiagonalQuatCost(self.W(k), self.Rd, -self.W(k) * x[k], -self.Rd * u[k], 0.0, 1.0, q_ref[k], terminal=(k == N - 1)) for k in range(N)]

    def _build(self, lib, rows, costs, variant):
        p = T.Problem(T.Quadrotor(), T.Objective(costs), np.zeros(13), self.tf, constraints=_constraints(variant, self.N), batch=len(rows), lib=lib)
        p.set_initial_state(self.x0[rows])
        T.initial_controls(p, self.uf)
        return p

    def problem(self, lib, rows=None, variant="free"):
        rows = np.arange(self.B) if rows is None else np.asarray(rows)
        xi = np.zeros(13); xi[3] = 1.0; xi[:3] = [0.1, 0.1, 0.1]
        N = self.N
        return self._build(lib, rows, self._costs(np.tile(xi, (N, 1)), np.tile(self.uf, (N, 1)), np.tile(IDENTITY, (N, 1))), variant)

    def window(self, start, k):
        return np.minimum(np.asarray(start, dtype=np.int64) - 1 + k, self.Nref - 1)

    def single(self, lib, b, start=None, variant="free", attitude=True):
        j = self.window(self.start[b] if start is None else start, np.arange(self.N))
        x = self.Xref[b, j]
        return self._build(lib, [b], self._costs(x, self.Uref[b, j], x[:, 3:7] if attitude else np.tile(IDENTITY, (self.N, 1))), variant)

    def feed_by_recipe(self, p, start, rows=None, attitude=True):
        """The host recipe: N ``set_cost_linear_batch`` calls with q_b = -Q x_ref[j], r_b = -R u_ref[j] (numpy rounds every product on its
        own) plus N ``set_cost_attitude_batch`` calls with the gathered quaternions."""
        rows = np.arange(self.B) if rows is None else np.asarray(rows)
        for k in range(self.N):
            j = self.window(start, k)
            cid = int(p._cost_index[k])
            x, u = self.Xref[rows, j], self.Uref[rows, j]
            p._call("set_cost_linear_batch", cid, p._pd(np.ascontiguousarray(-(self.W(k)[None, :] * x))), p._pd(np.ascontiguousarray(-(self.Rd[None, :] * u))))
            if attitude:
                T.set_cost_attitude_batch(p, cid, np.ascontiguousarray(x[:, 3:7]))


def phases(p):
    """The steps and the fields of cost_weight_fleets.phases, and with them: the rotational rows of the error-state gradient and the
    rotational block of the error-state Hessian (``qx_rot`` [B, N, 3], ``Qxx_rot`` [B, N, 3, 3] — where a Quadrotor's q_ref enters the
    expansion: -+ w G(q)'q_ref and the curvature term -(q'g) I that the attitude Jacobian adds), and the trajectory the forward pass
    accepted (with TRAJOPT_ACCEPT_ROLL_MIN=1: re-rolled, the cost evaluated again)."""
    from trajopt_amd import internal as I
    T.rollout(p)
    if len(p.constraints):
        I.dual_update(p); I.dual_update(p)
    r = SimpleNamespace(J=T.cost(p), Jk=T.stage_costs(p), al=I.al_cost(p) if len(p.constraints) else T.cost(p))
    r.grad, r.hess = I.cost_gradient_hessian(p)
    I.expand(p)
    e = I.cost_expansion(p)
    r.E = np.concatenate([np.asarray(e[k]).reshape(p.B, -1) for k in ("Qxx", "Quu", "Qux", "qx", "qu")], axis=1)
    r.qx_rot, r.Qxx_rot = np.array(e["qx"][:, :, 3:6]), np.array(e["Qxx"][:, :, 3:6, 3:6])
    I.backwardpass(p)
    g = I.gains(p)
    r.K, r.d = g["K"], g["d"]
    r.ls, r.Jn = I.forwardpass(p)
    r.X, r.U = T.states(p), T.controls(p)
    return r


_cache = {}


def goal(B):
    if ("goal", B) not in _cache:
        _cache["goal", B] = GoalFleet(B)
    return _cache["goal", B]


def tracking(B):
    if ("tracking", B) not in _cache:
        _cache["tracking", B] = TrackingFleet(B)
    return _cache["tracking", B]


def _singles(name, B, solver, b, attitude=True):
    v = variant_of(solver)
    return goal(B).single(_oracle(), b, v, attitude) if name == "goal" else tracking(B).single(_oracle(), b, None, v, attitude)


def _oracle():
    from oracle_binding import load_oracle
    return load_oracle()


def reference_phases(B, variant):
    """The phases of the goal fleet's B singles, stacked."""
    key = ("phases", B, variant)
    if key not in _cache:
        f = goal(B)
        _cache[key] = F._stack([phases(f.single(_oracle(), b, variant)) for b in range(B)])
    return _cache[key]


def reference_solve(name, B, solver, ulps=0, attitude=True):
    """The B singles of fleet ``name`` solved with ``solver`` ("ilqr" on the free variant, "al" / "altro" on the bound one), stacked;
    ``ulps``: from inputs moved by that many units in the last place; ``attitude=False``: with the shared (goal) / identity (tracking) q_ref."""
    key = ("solve", name, B, solver, ulps, attitude)
    if key not in _cache:
        Solver, kw = SOLVERS[solver]
        ps = [_singles(name, B, solver, b, attitude) for b in range(B)]
        _cache[key] = solve_singles([ulp_moved(p, ulps) if ulps else p for p in ps], Solver, kw)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ combination: attitudes + weights + goals + limits
COMBO_B = 24


def combo():
    """The goal fleet (B = 24) with, per trajectory, its own diagonal weights (nominal times 10^U(-0.5, 0.5) per entry, as in
    cost_weight_fleets) and its own upper control limit U(2.5, 3.5): -> SimpleNamespace(Q, R, Qf [B, .], u_max [B])."""
    if "combo" not in _cache:
        g, rng = goal(COMBO_B), np.random.default_rng(413)
        _cache["combo"] = SimpleNamespace(Q=g.Q0 * F.spread(rng, (COMBO_B, 13)), R=g.R0 * F.spread(rng, (COMBO_B, 4)), Qf=g.Qf0 * F.spread(rng, (COMBO_B, 13)),
                                          u_max=rng.uniform(2.5, 3.5, COMBO_B))
    return _cache["combo"]


def combo_single(lib, b):
    """Trajectory b alone with everything in its descriptors (and the nominal constants c, which no setter touches)."""
    g, c = goal(COMBO_B), combo()
    xf, uf = g.Xf[b], g.uf
    c0 = 0.5 * g.xf @ (g.Q0 * g.xf) + 0.5 * uf @ (g.R0 * uf)
    cf0 = 0.5 * g.xf @ (g.Qf0 * g.xf) + 0.5 * uf @ (g.R0 * uf)
    stage = T.DiagonalQuatCost(c.Q[b], c.R[b], -c.Q[b] * xf, -c.R[b] * uf, c0, 1.0, xf[3:7])
    term = T.DiagonalQuatCost(c.Qf[b], c.R[b], -c.Qf[b] * xf, -c.R[b] * uf, cf0, 1.0, xf[3:7], terminal=True)
    cons = T.ConstraintList(13, 4, g.N)
    T.add_constraint(cons, T.BoundConstraint(13, 4, u_min=0.0, u_max=c.u_max[b]), range(1, g.N))
    p = T.Problem(T.Quadrotor(), T.Objective(stage, term, g.N), np.zeros(13), g.tf, xf=xf, constraints=cons, batch=1, lib=lib)
    p.set_initial_state(configs.quadrotor_x0(1, b))
    T.initial_controls(p, uf)
    return p


def combo_batch(lib):
    g, c = goal(COMBO_B), combo()
    p = g.shared(lib, "bound")
    T.set_goal_state(p, np.array(g.Xf), objective=False, constraint=False, attitude=True)      # the attitudes alone ...
    T.set_LQR_weights_batch(p, c.Q, c.R, c.Qf, xf=np.array(g.Xf), uf=g.uf)                      # ... the weights and the goals' linear terms ...
    T.set_bounds_batch(p, 0, u_max=np.tile(c.u_max[:, None], (1, 4)), u_min=np.zeros((COMBO_B, 4)))   # ... and the limits
    return p


def combo_reference(solver="altro", ulps=0):
    key = ("combo", solver, ulps)
    if key not in _cache:
        Solver, kw = SOLVERS[solver]
        ps = [combo_single(_oracle(), b) for b in range(COMBO_B)]
        _cache[key] = solve_singles([ulp_moved(q, ulps) if ulps else q for q in ps], Solver, kw)
    return _cache[key]
