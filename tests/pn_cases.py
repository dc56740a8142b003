"""Projected-Newton polish cases away from the tuned shapes: a ladder of block strides NB = ne + candidate rows over the limits that
choose the kernel's code paths (csrc/k_pn.h: register / generic Cholesky, staged / unstaged solve sweeps, staged / unstaged factor
sweep, PN_NB_LIMIT), and batches in which some trajectories leave the polish by each of its exits next to healthy ones.

No AL solve in front: every start is a trajectory that is feasible by construction (Quadrotor at hover; Cartpole and double integrators
on a rollout of constant controls, or at rest), perturbed by a seeded normal.  The constraint data comes from that trajectory: goal and
waypoint targets are its states, linear equalities have b = A z_nominal, the control bounds that are meant to be active sit exactly on
the nominal control, and everything else is so wide that it stays a candidate row that never comes near active_set_tolerance_pn.

Shared by tests/test_pn_cases_oracle.py (vets every case on the CPU oracle alone), tests/test_pn_host.py (the kernel source compiled
for the host) and tests/test_gpu_pn_blocks.py (the GPU).  No GPU is needed to import this module."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np

import trajopt_amd as T
from trajectoryoptimization_jl_amd import configs
from failure_cases import shift_ulp

ROOT = Path(__file__).resolve().parent.parent
S = T.capi

# ------------------------------------------------------------------------------------------- the kernel source on the host
_host = None


def host_library():
    """tests/host_shim/pn_harness.cpp (the kernel source with TO_PN_HOST) as a shared library, built once under tests/host_shim/build."""
    global _host
    if _host is None:
        src = ROOT / "tests" / "host_shim" / "pn_harness.cpp"
        csrc = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
        so = ROOT / "tests" / "host_shim" / "build" / "libpn_host.so"
        deps = [src] + sorted(csrc.glob("*.h"))
        if not so.exists() or any(d.stat().st_mtime > so.stat().st_mtime for d in deps):
            so.parent.mkdir(exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(src.parent), "-I", str(csrc),
                            "-o", str(so), str(src)], check=True)
        lib = C.CDLL(str(so))
        lib.pn_host_solve.restype = C.c_int
        lib.pn_host_last_error.restype = C.c_char_p
        _host = lib
    return _host


def limits():
    """-> dict(nbr, pf, nb_limit, max_rows): PN_NBR, PN_PF, PN_NB_LIMIT, PN_MAX_ROWS of the kernel source (pn_host_limits)."""
    v = [C.c_int(0) for _ in range(4)]
    host_library().pn_host_limits(*[C.byref(x) for x in v])
    return dict(zip(("nbr", "pf", "nb_limit", "max_rows"), (x.value for x in v)))


def rungs(ne, nc):
    """The strides of the ladder for a model with ne error-state and nc = ne + m step coordinates, from the kernel's own limits: the last
    register-Cholesky / staged-solve stride and the first generic one, the last staged and the first unstaged factor sweep, the last
    launch whose dynamic LDS stays within 64 KiB is found by the caller (it depends on pn_lds_doubles), the limit."""
    L = limits()
    reg = min(L["nbr"], math.isqrt(64 * L["pf"]))
    fac = ne + (64 * L["pf"]) // nc
    return dict(last_reg=reg, first_generic=reg + 1, last_staged_factor=min(fac, L["nb_limit"]), first_unstaged_factor=fac + 1, limit=L["nb_limit"])


def lds_bytes(ne, m, NB):
    """8 * pn_lds_doubles<M>(NB) (csrc/k_pn.h): the dynamic LDS of a polish launch."""
    nc = ne + m
    ncp = nc | 1
    return 8 * (3 * NB * NB + ne * NB + 2 * ne * ncp + 3 * (NB - ne) * ncp + 2 * nc + 2 * NB + 64)


# ------------------------------------------------------------------------------------------------------------- nominal trajectories
def _rollout(model, x0, u, N, tf):
    """[N, n]: the oracle's rollout of the constant control u from x0."""
    from oracle_binding import load_oracle
    n, m = model.dims()
    obj = T.LQRObjective(np.ones(n), np.ones(m), np.ones(n), np.zeros(n), N, checks=False)
    p = T.Problem(model, obj, np.asarray(x0, dtype=np.float64), tf, constraints=T.ConstraintList(n, m, N), batch=1, lib=load_oracle())
    T.initial_controls(p, np.asarray(u, dtype=np.float64))
    T.rollout(p)
    return T.states(p)[0]


def _filler(n, m, count, z, big=50.0, states_only=False):
    """`count` candidate rows that never come near their bound: wide state bounds first, LinearConstraint inequality rows for a third of
    them (and for whatever two bounds per state cannot hold)."""
    out = []
    nlin = count // 3
    nbd = count - nlin
    if nbd > 2 * n:
        nlin, nbd = nlin + nbd - 2 * n, 2 * n
    if nbd:
        hi, lo = np.full(n, np.inf), np.full(n, -np.inf)
        hi[:min(nbd, n)] = z[:min(nbd, n)] + big
        if nbd > n:
            lo[:nbd - n] = z[:nbd - n] - big
        out.append(T.BoundConstraint(n, m, x_max=hi, x_min=lo))
    if nlin:
        w = n if states_only else n + m
        A = np.zeros((nlin, w))
        for r in range(nlin):
            A[r, r % w] += 1.0
            A[r, (r + 3) % w] -= 0.5
        chunk = min(S.TO_MAX_P, S.TO_MAX_CON_PARAMS // (w + 1))   # rows one descriptor holds
        for r0 in range(0, nlin, chunk):
            Ar = A[r0:r0 + chunk]
            out.append(T.LinearConstraint(n, m, Ar, Ar @ z[:w] + big, T.Inequality(), inds=range(1, w + 1)))
    assert sum(c.p for c in out) == count
    return out


class PnCase:
    """One batch for the polish.  ``cons``: [(constraint, k1, k2)] (1-based knots); ``Xn`` / ``Un``: the nominal trajectory [N, n] /
    [N-1, m]; ``scale``: [B] perturbation scale of every trajectory (states; controls take a fifth of it, so that a control bound placed
    on the nominal control stays within active_set_tolerance_pn); ``NB`` / ``nb``: the stride and the largest active block the case is
    built to hit (the tests recompute both); ``opts``: solver options; ``expect``: exit classes the oracle must show (see classify);
    ``tol``: tolerance on X / U / c_max of the trajectories that end PROJECTION_FAIL — 16 x the oracle's own spread over +-1 ulp starts
    and its two factorisation orders, measured by tests/test_pn_cases_oracle.py (None: every trajectory converges); ``edit``: last
    changes to the start (X, U) -> None, e.g. a NaN."""

    def __init__(self, name, model, tf, cons, Xn, Un, scale, NB, nb, seed=1, opts=None, expect=(), tol=None, edit=None, terminal_nb=None,
                 cost=None):
        self.name, self.model, self.tf, self.cons, self.Xn, self.Un = name, model, tf, cons, Xn, Un
        self.scale, self.NB, self.nb, self.seed, self.opts, self.expect, self.tol, self.edit = np.asarray(scale, dtype=np.float64), NB, nb, seed, dict(opts or {}), tuple(expect), tol, edit
        self.terminal_nb, self.cost = terminal_nb, cost
        self.N, self.B = Xn.shape[0], self.scale.size
        self._start = None

    def start(self):
        """(X [B, N, n], U [B, N-1, m]): the same arrays for every library"""
        if self._start is None:
            rng = np.random.default_rng(self.seed)
            X = self.Xn[None] + self.scale[:, None, None] * rng.normal(size=(self.B,) + self.Xn.shape)
            U = self.Un[None] + 0.2 * self.scale[:, None, None] * rng.normal(size=(self.B,) + self.Un.shape)
            X[:, 0] = self.Xn[0]     # the initial condition holds (its rows are part of every block all the same)
            if self.edit:
                self.edit(X, U)
            self._start = (X, U)
        return self._start

    def build(self, lib, ulp=0, sel=None, model=None, **extra):
        """The problem on ``lib`` with the start loaded (``ulp``: every entry of it moved by that many representable numbers; ``sel``:
        only these trajectories of the batch)."""
        n, m = self.model.dims()
        N = self.N
        if self.cost is not None:
            obj = self.cost(N)
        else:
            obj = T.LQRObjective(np.ones(n), np.full(m, 0.1), np.full(n, 10.0), self.Xn[-1], N, checks=False)
        cl = T.ConstraintList(n, m, N)
        for con, k1, k2 in self.cons:
            T.add_constraint(cl, con, (k1, k2))
        kw = dict(self.opts)
        kw.update(extra)
        o = T.SolverOptions(lib=lib, **kw)
        X, U = self.start()
        sel = np.arange(self.B) if sel is None else np.asarray(sel)
        p = T.Problem(model or self.model, obj, self.Xn[0], self.tf, xf=self.Xn[-1], constraints=cl, batch=len(sel), lib=lib, options=o)
        X, U = X[sel], U[sel]
        if ulp:
            X, U = shift_ulp(X, ulp), shift_ulp(U, ulp)
        T.initial_states(p, X)
        T.initial_controls(p, U)
        return p

    def polish(self, lib, ulp=0, sel=None, **extra):
        """-> dict(status, iterations_pn, c_max, cost, X, U, defect, prob) of to_pn_solve from the start"""
        p = self.build(lib, ulp, sel, **extra)
        s = T.ProjectedNewtonSolver(p).solve()
        return dict(status=s.stats["status"].copy(), iterations_pn=s.stats["iterations_pn"].copy(), c_max=s.stats["c_max"].copy(),
                    cost=s.stats["cost"].copy(), iterations=s.stats["iterations"].copy(), X=T.states(p), U=T.controls(p),
                    defect=T.dynamics_defect(p), prob=p)


def _options_of(prob):
    o = T.SolverOptions(lib=prob._lib)
    prob._call("get_options", C.byref(o._o))
    return o


def fleet_models(case, seed=4):
    """One plant per trajectory for a Cartpole case (tests/model_params_fleet.py draw_models: parameters within +-20 %, model 0 nominal)."""
    from model_params_fleet import draw_models
    return draw_models("cartpole", case.B, seed)


def polish_fleet(case, oracle, models, ulp=0):
    """The reference for per-trajectory plants: trajectory b polished by the oracle in a single-trajectory problem built on models[b]
    (the oracle knows nothing about per-trajectory parameters) -> the dict of PnCase.polish, stacked along the batch."""
    outs = [case.polish(oracle, ulp=ulp, sel=[b], model=models[b]) for b in range(case.B)]
    res = {k: np.concatenate([o[k] for o in outs]) for k in outs[0] if k != "prob"}
    res["probs"] = [o["prob"] for o in outs]
    return res


def altro(case, lib, ulp=0, nan_control=None, sel=None):
    """to_altro_solve on the case: the AL stage starts from the case's controls (it rolls the states out itself), then the polish with
    the case's options.  ``nan_control``: (b, k) of a control entry set to NaN — a trajectory the AL stage must leave alone.
    -> the dict of PnCase.polish plus iterations_outer."""
    p = case.build(lib, ulp=ulp, sel=sel)
    if nan_control is not None:
        U = T.controls(p)
        U[nan_control[0], nan_control[1], 0] = np.nan
        T.initial_controls(p, U)
    s = T.ALTROSolver(p).solve()
    out = {k: s.stats[k].copy() for k in ("status", "iterations", "iterations_outer", "iterations_pn", "c_max", "cost")}
    out.update(X=T.states(p), U=T.controls(p), prob=p)
    return out


# the exit cases that also go through to_altro_solve, with the control entry that is NaN
ALTRO = {"budget_n_steps0": None, "nan_state": (2, 5)}
# the cases that also run with one plant per trajectory (a ladder rung at a generic-path stride and an exit case; Cartpole)
FLEET = ("cartpole_rest_NB26", "nan_state")


def strides(case, prob):
    """(NB, nb [N]) recomputed from the library's own evaluate_constraints at the problem's current trajectories: NB = ne + the most
    candidate rows on a knot; nb[k] = ne + the most active rows of knot k over the batch (equalities; inequalities within
    active_set_tolerance_pn; rows of control bounds never at the terminal knot, where their gradient vanishes)."""
    n, m = case.model.dims()
    ne, N = case.model.errstate_dim, case.N
    cand, act = np.zeros(N, int), np.zeros((prob.B, N), int)
    tol = _options_of(prob).active_set_tolerance_pn
    for i, (con, k1, k2) in enumerate(case.cons):
        v = T.evaluate_constraints(prob, i)             # [B, nk, p]
        rows = 1 if isinstance(con.sense(), T.SecondOrderCone) else con.p
        cand[k1 - 1:k2] += rows
        if isinstance(con.sense(), T.Equality):
            a = np.ones(v.shape, bool)
        else:
            a = v >= -tol
        if isinstance(con, T.BoundConstraint):           # rows: finite upper bounds of [x; u], then finite lower ones
            is_u = np.array([(j - 1) % (n + m) >= n for j in con.inds])
            for j, k in enumerate(range(k1 - 1, k2)):
                if k == N - 1:
                    a[:, j, is_u] = False
        act[:, k1 - 1:k2] += a.sum(axis=2)
    return ne + int(cand.max()), ne + act.max(axis=0), ne + cand


def classify(case, out, oracle_prob):
    """-> [B] sets of exit classes from the oracle's polish trace (oracle_binding.pn_trace) and its result:
    "converged", "budget" (n_steps + 1 linearisations spent above tolerance), "factor" (a pivot was not positive), "linesearch" (a
    projection ended with every trial step size rejected), "rate" (a projection ended by the convergence-rate break), "nan"."""
    from oracle_binding import pn_trace
    n_steps = _options_of(oracle_prob).n_steps
    labels = []
    for b in range(oracle_prob.B):
        tr = pn_trace(oracle_prob, b)
        L = set()
        assert len(tr) == out["iterations_pn"][b]
        if out["status"][b] == S.SOLVE_SUCCEEDED:
            L.add("converged")
        if np.isnan(out["c_max"][b]):
            L.add("nan")
        for _, _, why in tr:
            if why in ("factor", "linesearch", "rate"):
                L.add(why)
        if out["status"][b] != S.SOLVE_SUCCEEDED and len(tr) == n_steps + 1 and "factor" not in L and "nan" not in L:
            L.add("budget")
        labels.append(L)
    return labels


def assert_case_matches(case, got, ref, what):
    """got / ref: dicts of status, iterations_pn, c_max, X, U (and cost, defect where both have them).  Integers bit-exact; converged
    trajectories at the tolerances of tests/test_gpu_pn.py test_pn_solve_vs_oracle (X / U 1e-8, c_max 1e-9, cost 1e-9 relative, defect
    1e-10 + 1e-3 relative); the ones that end PROJECTION_FAIL at the case's own tolerance (16 x the oracle's spread, TOL), NaN where the
    oracle has NaN.  Every figure is printed before it is asserted."""
    B = ref["status"].size
    ok = ref["status"] == S.SOLVE_SUCCEEDED
    keys = [k for k in ("X", "U", "c_max", "cost", "defect") if k in got and k in ref]
    for k in keys:
        err = np.abs(got[k] - ref[k]).reshape(B, -1)
        worst = lambda e: float(np.nanmax(e)) if e.size and not np.all(np.isnan(e)) else 0.0
        print(f"{what} {case.name} {k}: largest difference {worst(err[ok]):.3e} (converged), {worst(err[~ok]):.3e} (PROJECTION_FAIL, tolerance {case.tol})")
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=f"{what}: status")
    np.testing.assert_array_equal(got["iterations_pn"], ref["iterations_pn"], err_msg=f"{what}: iterations_pn")
    conv = dict(X=(0, 1e-8), U=(0, 1e-8), c_max=(1e-3, 1e-9), cost=(1e-9, 0), defect=(1e-3, 1e-10))
    for k in keys:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), f"{what}: NaN pattern of {k}"
        np.testing.assert_allclose(got[k][ok], ref[k][ok], rtol=conv[k][0], atol=conv[k][1], err_msg=f"{what}: {k}, converged")
        if (~ok).any():
            np.testing.assert_allclose(got[k][~ok], ref[k][~ok], rtol=1e-9 if k == "cost" else 0, atol=case.tol, equal_nan=True,
                                       err_msg=f"{what}: {k}, PROJECTION_FAIL")


# ------------------------------------------------------------------------------------------------------------------------ builders
def _quad_cost(xh, uh):
    def cost(N):
        Qd = np.array([1.0, 1, 1, 0, 0, 0, 0, .1, .1, .1, .1, .1, .1])
        Rd = np.full(4, 1e-2)
        return T.Objective(T.QuatLQRCost(Qd, Rd, xh, uh, w=1.0), T.QuatLQRCost(100.0 * Qd, Rd, xh, uh, w=1.0, terminal=True), N)
    return cost


def quadrotor_rung(NB, full_at, N=11, B=3, waypoint=False, term_quatvec=True, seed=1, scale=1e-3, name=None, dup_goal=False, goal_shift=0.0, **kw):
    """Quadrotor at hover (ne = 12, nc = 16).  Terminal knot: Goal on position and velocities (9) [+ QuatVecEq (3)]; control bounds on
    the hover control on two mid-horizon knots (4 active rows each); ``waypoint``: Goal + QuatVecEq on the first of them (nb = 28
    there); inactive filler rows on knot ``full_at`` (0-based) bring its stride to NB."""
    model = T.Quadrotor()
    n, m = model.dims()
    uh = model.hover_control()
    xh = model.build_state([0.3, -0.2, 0.5])
    Xn, Un = np.tile(xh, (N, 1)), np.tile(uh, (N - 1, 1))
    z = np.r_[xh, uh]
    kw_ = N // 2                      # 1-based knot of the waypoint / first saturated control
    cons = [(T.BoundConstraint(n, m, u_max=uh), kw_, kw_ + 1)]
    per = {kw_ - 1: 4, kw_: 4}
    if waypoint:
        cons += [(T.GoalConstraint(xh, configs.C5_GOAL_INDS), kw_, kw_), (T.QuatVecEq(n, m, xh[3:7]), kw_, kw_)]
        per[kw_ - 1] += 12
    xg = xh.copy()
    xg[0] += goal_shift                 # (beyond_cases: a goal the AL stage has to work for, so that it leaves something to polish)
    cons.append((T.GoalConstraint(xg, configs.C5_GOAL_INDS), N, N))
    per[N - 1] = 9
    if dup_goal:
        cons.append((T.GoalConstraint(xh, configs.C5_GOAL_INDS), N, N))
        per[N - 1] += 9
    if term_quatvec:
        cons.append((T.QuatVecEq(n, m, xh[3:7]), N, N))
        per[N - 1] += 3
    fill = NB - 12 - per.get(full_at, 0)
    assert fill >= 0 and all(12 + v <= NB for v in per.values()), (NB, per)
    for c in _filler(n, m, fill, z, states_only=(full_at == N - 1)):
        cons.append((c, full_at + 1, full_at + 1))
    nb = 12 + max(16 if waypoint else 4, per[N - 1])     # (the terminal rows counted so far are all equalities)
    return PnCase(name or f"quadrotor_NB{NB}", model, 0.2 * (N - 1), cons, Xn, Un, np.full(B, scale), NB, nb, seed=seed, cost=_quad_cost(xh, uh),
                  terminal_nb=12 + per[N - 1], **kw)


def small_rung(name, model, x0, u, NB, N, B, tf, waypoint_inds, seed=1, scale=None, linear_eq=False, circle=None, at_rest=False, **kw):
    """A small model on the rollout of the constant control u from x0 (``at_rest``: x0 is an equilibrium under u, the trajectory stays
    there).  Goal on the whole terminal state; the control bound on the nominal control over a mid-horizon range (active); a waypoint
    Goal on ``waypoint_inds`` inside it; ``linear_eq``: two LinearConstraint equality rows b = A z_nominal on one more knot; inactive
    filler rows on the waypoint knot bring the stride to NB."""
    n, m = model.dims()
    x0, u = np.asarray(x0, dtype=np.float64), np.asarray(u, dtype=np.float64)
    Xn = np.tile(x0, (N, 1)) if at_rest else _rollout(model, x0, u, N, tf)
    Un = np.tile(u, (N - 1, 1))
    kw_ = N // 2
    cons = [(T.BoundConstraint(n, m, u_max=u), kw_ - 1, kw_ + 1), (T.GoalConstraint(Xn[kw_ - 1], waypoint_inds), kw_, kw_)]
    rows = m + len(waypoint_inds)
    if linear_eq:
        A = np.random.default_rng(5).normal(size=(2, n + m))
        zk = np.r_[Xn[kw_ + 2], u]
        cons.append((T.LinearConstraint(n, m, A, A @ zk, T.Equality()), kw_ + 3, kw_ + 3))
    if circle is not None:
        cons.append(circle)
        rows_inactive = circle[0].p if circle[1] <= kw_ <= circle[2] else 0
    else:
        rows_inactive = 0
    cons.append((T.GoalConstraint(Xn[-1]), N, N))
    for c in _filler(n, m, NB - n - rows - rows_inactive, np.r_[Xn[kw_ - 1], u]):
        cons.append((c, kw_, kw_))
    scale = np.full(B, 1e-3) if scale is None else scale
    return PnCase(name, model, tf, cons, Xn, Un, scale, NB, n + max(rows, n), seed=seed, **kw)


def _nan_edit(b, k):
    def edit(X, U):
        X[b, k, 1] = np.nan
    return edit


def _circle_centre_edit(bs, k):
    """trajectories bs stand 1e-160 off the circle's centre at knot k: the row is active (value r^2), its gradient 2e-160 has a positive
    squared norm, and its diagonal entry of S, (g W) g with W ~ 1e-6, is exactly 0.0 on every side: with rho_chol = 0 the pivot is not
    positive.  (A row whose gradient IS zero — a LinearConstraint row with a zero A row — never gets that far: rows with a vanishing
    gradient are left out of the active set, in the oracle and in the kernel alike.)"""
    def edit(X, U):
        for b in bs:
            X[b, k, 0:2] = 1e-160
    return edit


def beyond_cases():
    """Outside what the polish takes (op_pn_prepare refuses; to_altro_solve keeps the AL result): a Quadrotor stride of PN_NB_LIMIT + 1,
    and more than PN_MAX_ROWS candidate rows on one knot of the 1-D double integrator."""
    L = limits()
    return [quadrotor_rung(L["nb_limit"] + 1, 4, waypoint=True, name="quadrotor_beyond_nb_limit", goal_shift=0.3),
            small_rung("dint1_beyond_max_rows", T.DoubleIntegrator(1.0, 1), [0.2, 0.0], [0.3], 2 + L["max_rows"] + 1, 11, 4, 1.0, [1])]


CASES = {}
LADDER, EXITS = [], []
GUARD = []          # the cases that also run under TRAJOPT_GUARD=1: the limit on the Cartpole, the last launch within 64 KiB of LDS, the NaN


def _add(case, where):
    CASES[case.name] = case
    where.append(case.name)
    return case


def _build_all():
    q = rungs(12, 16)
    lim = q["limit"]
    kib64 = max(NB for NB in range(13, lim + 1) if lds_bytes(12, 4, NB) <= 65536)
    # ---- the ladder on the Quadrotor.  Fullest knot: 1, mid-horizon (the waypoint) or N-1, knots without any candidate row next to it
    _add(quadrotor_rung(q["last_reg"], 10, term_quatvec=False), LADDER)                     # 21: the fullest knot is the terminal one (C5's shape)
    _add(quadrotor_rung(q["first_generic"], 1, term_quatvec=False), LADDER)                 # 22: fullest at knot 1, nothing on knots 0 and 2
    _add(quadrotor_rung(q["first_generic"] + 2, 10), LADDER)                                # 24: C5', Goal(9) + QuatVecEq(3) at the terminal knot
    _add(quadrotor_rung(32, 4, waypoint=True), LADDER)
    _add(quadrotor_rung(q["last_staged_factor"], 4, waypoint=True), LADDER)                 # 40
    _add(quadrotor_rung(q["first_unstaged_factor"], 1, waypoint=True), LADDER)              # 41: fullest at knot 1
    _add(quadrotor_rung(kib64, 4, waypoint=True), LADDER)                                   # 42: the last launch within 64 KiB of LDS
    _add(quadrotor_rung(lim - 1, 10, waypoint=True), LADDER)                                # 43: fullest at the terminal knot
    _add(quadrotor_rung(lim, 4, waypoint=True), LADDER)                                     # 44
    # ---- one rung each on the small models (other ne / nc / ncp in every index expression), and a horizon above 64 knots
    cp = T.Cartpole()
    _add(small_rung(f"cartpole_NB{lim}", cp, np.zeros(4), [0.4], lim, 13, 5, 1.2, [1, 3]), LADDER)
    _add(small_rung("dint3_NB31", T.DoubleIntegrator(1.0, 3), [0.2, -0.1, 0.3, 0, 0, 0], [0.3, -0.2, 0.1], 31, 15, 4, 1.4, [1, 2, 3, 5],
                    linear_eq=True), LADDER)
    _add(small_rung("cartpole_N70_NB23", cp, np.zeros(4), [0.15], 23, 70, 3, 3.45, [1, 2]), LADDER)
    _add(small_rung(f"cartpole_rest_NB{q['first_generic'] + 4}", cp, np.zeros(4), [0.0], q["first_generic"] + 4, 13, 6, 1.2, [1, 3], at_rest=True), LADDER)
    # ---- exits, each next to healthy trajectories
    big = np.array([1e-3, 0.3, 1e-3, 0.5, 1e-3, 0.2, 0.4])
    _add(small_rung("budget_n_steps0", cp, np.zeros(4), [0.4], 26, 13, 7, 1.2, [1, 3], scale=big, opts=dict(n_steps=0), expect=("budget", "converged"),
                    tol=TOL.get("budget_n_steps0")), EXITS)
    _add(small_rung("budget_n_steps1", cp, np.zeros(4), [0.4], 26, 13, 7, 1.2, [1, 3], scale=3.0 * big, opts=dict(n_steps=1), expect=("budget", "converged"),
                    tol=TOL.get("budget_n_steps1")), EXITS)
    di2 = T.DoubleIntegrator(1.0, 2)
    circle = (T.CircleConstraint(4, [0.0], [0.0], [0.5]), 3, 9)
    heavy = lambda N: T.LQRObjective(np.array([1e6, 1e6, 1.0, 1.0]), np.full(2, 0.1), np.full(4, 10.0), np.zeros(4), N, checks=False)
    _add(small_rung("zero_pivot", di2, [2.0, 1.0, 0.3, 0.2], [0.2, 0.1], 24, 11, 6, 1.0, [1, 2], circle=circle, opts=dict(rho_chol=0.0),
                    edit=_circle_centre_edit((1, 4), 6), cost=heavy, expect=("factor", "converged"), tol=TOL.get("zero_pivot")), EXITS)
    _add(small_rung("nan_state", cp, np.zeros(4), [0.4], 26, 13, 5, 1.2, [1, 3], edit=_nan_edit(2, 5), expect=("nan", "converged"),
                    tol=TOL.get("nan_state")), EXITS)
    _add(small_rung("rate_and_linesearch", cp, np.zeros(4), [0.4], 26, 13, 8, 1.2, [1, 3], seed=SEARCH["seed"], scale=SEARCH["scale"],
                    opts=dict(n_steps=3), expect=("rate", "linesearch"), tol=TOL.get("rate_and_linesearch")), EXITS)
    GUARD.extend([f"cartpole_NB{lim}", f"quadrotor_NB{kib64}", "nan_state"])
    # the same Goal twice at the terminal knot: S is singular but for rho_chol.  Every trajectory converges (reg_solve refines against
    # the unregularised S) and the oracle's spread is 1e-15, so the case stays, at the 1e-8 of the converged trajectories
    if "dependent_rows" not in DROPPED:
        _add(quadrotor_rung(42, 10, dup_goal=True, name="dependent_rows", opts=dict(rho_chol=1e-8), tol=TOL.get("dependent_rows")), EXITS)


# Tolerances of the trajectories that end PROJECTION_FAIL (they are not contracted by Newton): 16 x the oracle's own spread of X, U and
# c_max over starts moved by +-1 ulp and over its banded / dense factorisation, floored at 1e-12, as tests/test_pn_cases_oracle.py
# measures and prints it (that test fails when a figure here is below 16 x what it measures).
# Measured: spread 3.1e-13 (budget_n_steps0), 6.6e-12 (budget_n_steps1), 4.4e-16 (zero_pivot: the start is handed back), 5.6e-17 (nan_state).
TOL = dict(budget_n_steps0=5e-12, budget_n_steps1=1.1e-10, zero_pivot=1e-12, nan_state=1e-12)
# the seed / scales at which the oracle shows a projection ended by the convergence-rate break and one with every trial step rejected
SEARCH = dict(seed=1, scale=np.array([1e-3, 0.05, 0.1, 0.2, 0.3, 0.5, 0.8, 1.2]))
# cases the vetting removed, with the reason
DROPPED = {}

_build_all()
