"""Solver options off their defaults: rows (base batch, options both runs share, the override under test) over the batches of
tests/failure_cases.py and tests/pn_cases.py, plus a constrained Quadrotor with its second-order cone, and three restatements of what
the options mean that do not go through any solver code (step sizes, regularisation ladder, dual update).

Shared by tests/test_option_cases_oracle.py (which vets every row on the CPU oracle alone: the option bites, the clamps bind, every
integer survives last-bit changes of the inputs, the restatements hold) and tests/test_gpu_options.py (which runs the rows on every
kernel path).  No GPU is needed to import this module."""
import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs
import failure_cases as F
import pn_cases as PN

INTS = ("status", "iterations", "iterations_outer", "iterations_pn")
SOLVERS = {"ilqr": T.iLQRSolver, "al": T.ALSolver, "altro": T.ALTROSolver, "pn": T.ProjectedNewtonSolver}
# the narrow acceptance window of cartpole_no_progress: failed searches from the first pass on
WINDOW = dict(iterations_linesearch=2, line_search_lower_bound=0.3, line_search_upper_bound=0.95)


def _quadrotor_cone(B=24, N=41, tf=1.0, u_norm_max=2.6, **base):
    """The constrained Quadrotor (||u|| <= u_norm_max as a second-order cone on every knot, a goal constraint at the last): the cone
    duals are projected onto the cone, the goal duals are clamped to [-dual_max, dual_max]."""
    def build(lib, extra):
        o = F._options(lib, base, extra)
        p = configs.quadrotor_problem(batch=B, N=N, tf=tf, constrained=True, u_norm_max=u_norm_max, lib=lib, options=o)
        p.case_options = o
        return p
    return build


# (short inner solves: the oracle takes a second for 24 x 4 x 5 trajectory iterations)
QUADROTOR_CONE = F.Case("quadrotor_cone", _quadrotor_cone(iterations=5, iterations_outer=4), "al", expect=[], statuses=[], small=False)


class Row:
    """One option set.  ``case``: a failure_cases.Case (or a pn_cases.PnCase, ``solver == "pn"``: the polish alone from the case's
    start); ``shared``: options both runs have on top of the case's own; ``overrides``: the options under test, off their defaults;
    the BASE run is the same batch without ``overrides``.  ``late``: the row also runs with its overrides handed to a handle that
    was created without them."""

    def __init__(self, name, case, overrides, shared=None, late=False):
        self.name, self.case, self.overrides, self.shared, self.late = name, case, dict(overrides), dict(shared or {}), late
        self.options = tuple(self.overrides)
        self.pn = isinstance(case, PN.PnCase)
        self.solver = "pn" if self.pn else case.solver
        self.quadrotor = isinstance(case.model, T.Quadrotor) if self.pn else not case.small
        self.base = case.name

    def opts(self, override=True, **extra):
        kw = dict(self.shared)
        if override:
            kw.update(self.overrides)
        kw.update(extra)
        return kw

    def build(self, lib, ulp=0, override=True, **extra):
        """-> the problem, created with the row's options (``p.case_options``)"""
        kw = self.opts(override, **extra)
        if not self.pn:
            return self.case.build(lib, ulp, **kw)
        p = self.case.build(lib, ulp, **kw)
        p.case_options = PN._options_of(p)
        return p

    def solve(self, lib, ulp=0, override=True, late=False, **extra):
        """-> (stats dict of copies + total_iterations, X, U, prob).  ``late``: the handle is created WITHOUT the overrides, the
        solver hands them over (to_set_options) in front of the solve."""
        p = self.build(lib, ulp, override and not late, **extra)
        s = SOLVERS[self.solver](p, **(self.overrides if late else {})).solve()
        st = {k: np.array(v).copy() for k, v in s.stats.items()}
        st["total_iterations"] = int(s.total_iterations)
        return st, T.states(p), T.controls(p), p

    def first_pass(self, lib, ulp=0, override=True):
        """rollout / expand / backwardpass / gains / forwardpass through the phase API, with the nominal controls kept."""
        p = self.build(lib, ulp, override)
        T.rollout(p)
        U0, X0, J0 = T.controls(p), T.states(p), I.al_cost(p)
        I.expand(p)
        I.backwardpass(p)
        g = I.gains(p)
        ls, J = I.forwardpass(p)
        return dict(prob=p, gains=g, rho=g["rho"].copy(), bpfail=g["rho"] > p.case_options.bp_reg_max, ls=ls, J=J, J0=J0, X0=X0, U0=U0,
                    X=T.states(p), U=T.controls(p), rho_after=I.gains(p)["rho"])

    def duals_after(self, lib, k, override=True):
        """k x I.dual_update from zero duals on the rollout of the initial controls -> dict(c: [constraint values [B, nk, p]],
        steps: [per call: [(lam, mu) per constraint]] with the state before the first call in front, prob)."""
        p = self.build(lib, 0, override)
        T.rollout(p)
        ncon = len(p.constraints)
        c = [T.evaluate_constraints(p, i) for i in range(ncon)]
        steps = [[I.get_duals(p, i) for i in range(ncon)]]
        for _ in range(k):
            I.dual_update(p)
            steps.append([I.get_duals(p, i) for i in range(ncon)])
        return dict(c=c, steps=steps, prob=p)


def final_duals(p):
    return [I.get_duals(p, i)[0] for i in range(len(p.constraints))]


def clampable(p, i):
    """The duals of constraint i are clamped by dual_max (every sense but the second-order cone, whose duals are projected)."""
    return not isinstance(p.constraints[i].sense(), T.SecondOrderCone)


def at_clamp(p, lams, dual_max):
    """-> [B] bool: the trajectory holds an equality / inequality dual with |lam| == dual_max exactly."""
    hit = np.zeros(p.B, bool)
    for i, lam in enumerate(lams):
        if clampable(p, i):
            hit |= (np.abs(lam) == dual_max).reshape(p.B, -1).any(axis=1)
    return hit


# ------------------------------------------------------------------------------------------------------------------- restatements
def alpha_of(f, i):
    """f**i by i successive multiplications (csrc/ls_round.h ls_alpha)."""
    al = 1.0
    for _ in range(int(i)):
        al = al * f
    return al


def assert_step_sizes(fp, f, what):
    """An accepted index i >= 0 means U_new[b, 0] - U_old[b, 0] == f**i d[b, 0]: at knot 0 the state deviation is exactly zero, so the
    feedback term vanishes.  8 ulp of max(|U_old|, |U_new|, |f**i d|) per entry: one multiply and one add, possibly fused, give at most
    2 ulp, the factor 4 is margin.  -> the accepted indices checked."""
    ls, d, U0, U1, dV, J0 = fp["ls"], fp["gains"]["d"], fp["U0"], fp["U"], fp["gains"]["dV"], fp["J0"]
    # (a stationary point reports index 0 with NO step; none of the rows holds one on its first pass, which is asserted here)
    assert not ((ls >= 0) & (-(dV[:, 0] + dV[:, 1]) <= 1e-12 * (1.0 + np.abs(J0)))).any(), f"{what}: a zero step on the first pass"
    idx = np.where(ls >= 0)[0]
    for b in idx:
        step = alpha_of(f, ls[b]) * d[b, 0]
        tol = 8 * np.finfo(np.float64).eps * np.maximum(np.maximum(np.abs(U0[b, 0]), np.abs(U1[b, 0])), np.abs(step))
        err = np.abs((U1[b, 0] - U0[b, 0]) - step)
        assert (err <= tol).all(), f"{what}: trajectory {b}, index {ls[b]}: U_new - U_old = {U1[b, 0] - U0[b, 0]}, f**i d = {step} (f = {f})"
    return ls[idx]


def reg_increase(o, rho, drho):
    """common.h reg_increase as the header documents it"""
    f = o.bp_reg_increase_factor
    drho = max(drho * f, f)
    return max(rho * drho, o.bp_reg_min), drho


def reg_decrease(o, rho, drho):
    f = o.bp_reg_increase_factor
    drho = min(drho / f, 1.0 / f)
    r = rho * drho
    return (r if r > o.bp_reg_min else 0.0), drho


def reg_ladder(o, rho0=None):
    """The regularisation a first backward pass can leave, from (bp_reg_initial, drho = 0): k = 0, 1, ... restarts, each one increase,
    then one decrease -> (passed: {rho: [the (rho, drho) states that show it]}, failed: the first level above bp_reg_max, which a failed
    pass reports)."""
    rho, drho = (o.bp_reg_initial if rho0 is None else rho0), 0.0
    passed = {}
    for k in range(400):
        if k:
            rho, drho = reg_increase(o, rho, drho)
        if rho > o.bp_reg_max:
            return passed, rho
        r, dr = reg_decrease(o, rho, drho)
        passed.setdefault(r, []).append((r, dr))
    raise AssertionError("the ladder does not reach bp_reg_max")


def assert_ladder(fp, o, what):
    """Every rho after the backward pass is bit-equal to a member of the ladder; after a failed search it is bit-equal to one more
    increase plus bp_reg_fp; every other trajectory keeps it.  -> (levels seen, failed searches)"""
    passed, failed = reg_ladder(o)
    rho, after, ls = fp["rho"], fp["rho_after"], fp["ls"]
    nfail = 0
    for b in range(rho.size):
        if rho[b] > o.bp_reg_max:
            assert rho[b] == failed and after[b] == rho[b] and ls[b] == -1, f"{what}: trajectory {b}: failed pass with rho {rho[b]}, ladder ends at {failed}"
            continue
        assert rho[b] in passed, f"{what}: trajectory {b}: rho {rho[b]!r} is no member of the ladder {sorted(passed)[:8]}..."
        if ls[b] >= 0:
            assert after[b] == rho[b], f"{what}: trajectory {b}: an accepted step changed rho"
        else:
            want = [reg_increase(o, r, dr)[0] + o.bp_reg_fp for r, dr in passed[rho[b]]]
            assert after[b] in want, f"{what}: trajectory {b}: rho {after[b]!r} after a failed search from {rho[b]!r}, wanted {want}"
            nfail += 1
    return sorted(set(rho.tolist())), nfail


def soc_projection(lb):
    """Projection of [v; s] onto the second-order cone (the oracle's dual_update / problem_dev.h con_dual_update), rows [..., p]."""
    v, s = lb[..., :-1], lb[..., -1]
    a = np.sqrt((v * v).sum(axis=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        cf = 0.5 * (1 + s / a)
    out = np.concatenate([v * cf[..., None], (a * cf)[..., None]], axis=-1)
    out = np.where((a <= s)[..., None], lb, out)
    return np.where((a <= -s)[..., None], 0.0, out)


def assert_dual_updates(du, o, what):
    """Each call of I.dual_update restated from the duals in front of it: mu' = min(mu scaling, penalty_max) exactly, lam' =
    clip(lam + mu c, -dual_max, dual_max) (equalities) / clip(lam + mu c, 0, dual_max) (inequalities) / the cone projection of lam - mu c
    at rtol 1e-12, atol 1e-13, entries at a clamp exactly +-dual_max; mu starts at penalty_initial, the duals at 0.
    -> ([B] the penalty clamp binds at the end, [B] a dual sits at its clamp at the end)"""
    p = du["prob"]
    B = p.B
    for i, (lam, mu) in enumerate(du["steps"][0]):
        assert (lam == 0).all() and (mu == o.penalty_initial).all(), f"{what}: constraint {i} does not start from zero duals and penalty_initial"
    for j in range(1, len(du["steps"])):
        for i, ((lam0, mu0), (lam1, mu1)) in enumerate(zip(du["steps"][j - 1], du["steps"][j])):
            np.testing.assert_array_equal(mu1, np.minimum(mu0 * o.penalty_scaling, o.penalty_max), err_msg=f"{what}: penalty of constraint {i}, call {j}")
            c, m = du["c"][i], mu0[:, None, None]
            sense = p.constraints[i].sense()
            if isinstance(sense, T.SecondOrderCone):
                want = soc_projection(lam0 - m * c)
            elif isinstance(sense, T.Equality):
                want = np.clip(lam0 + m * c, -o.dual_max, o.dual_max)
            else:
                want = np.clip(lam0 + m * c, 0.0, o.dual_max)
            np.testing.assert_allclose(lam1, want, rtol=1e-12, atol=1e-13, err_msg=f"{what}: duals of constraint {i}, call {j}")
            if not isinstance(sense, T.SecondOrderCone):
                hit = np.abs(want) == o.dual_max
                np.testing.assert_array_equal(lam1[hit], want[hit], err_msg=f"{what}: duals of constraint {i} at the clamp, call {j}")
                assert (np.abs(lam1) <= o.dual_max).all()
    last = du["steps"][-1]
    mu_bound = np.ones(B, bool)
    for lam, mu in last:
        mu_bound &= mu == o.penalty_max
    return mu_bound, at_clamp(p, [lam for lam, _ in last], o.dual_max)


# --------------------------------------------------------------------------------------------------------- what the oracle says
_cache = {}


def oracle_solve(row, oracle, override=True):
    key = ("solve", row.name, override)
    if key not in _cache:
        st, X, U, p = row.solve(oracle, override=override)
        _cache[key] = (st, X, U, final_duals(p), p.case_options)
    return _cache[key]


def oracle_first_pass(row, oracle):
    key = ("first", row.name)
    if key not in _cache:
        _cache[key] = row.first_pass(oracle)
    return _cache[key]


def oracle_duals(row, oracle, k):
    key = ("duals", row.name, k)
    if key not in _cache:
        _cache[key] = row.duals_after(oracle, k)
    return _cache[key]


def differs(row, oracle):
    """-> [B] bool: the override changes an integer of the trajectory's solve, or its states by more than 1e-9 relative."""
    st, X = oracle_solve(row, oracle)[:2]
    s0, X0 = oracle_solve(row, oracle, override=False)[:2]
    d = F.trajectory_error(X, X0) > 1e-9
    for k in INTS:
        d |= st[k] != s0[k]
    return d


def stability(row, oracle):
    """-> (mask [B]: every integer of the solve is the same and X, U, cost agree to 1e-8 between the oracle's run and each of its runs
    from starts moved by the steps of failure_cases.ULPS; unstable [B]: an integer changed).  The GPU is held to the VALUES of the
    masked trajectories only; computed on the oracle alone, once per row."""
    key = ("mask", row.name)
    if key not in _cache:
        st, X, U = oracle_solve(row, oracle)[:3]
        ok, unstable = np.ones(X.shape[0], bool), np.zeros(X.shape[0], bool)
        for ulp in F.ULPS:
            s2, X2, U2, _ = row.solve(oracle, ulp=ulp)
            for k in INTS:
                unstable |= s2[k] != st[k]
            ok &= F.trajectories_close(X2, X, 1e-8) & F.trajectories_close(U2, U, 1e-8)
            ok &= np.abs(s2["cost"] - st["cost"]) <= 1e-8 * np.maximum(1.0, np.abs(st["cost"]))
        _cache[key] = (ok & ~unstable, unstable)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------------------ the rows
ROWS = {}


def _row(name, case, overrides, **kw):
    ROWS[name] = Row(name, F.CASES[case] if isinstance(case, str) and case in F.CASES else case, overrides, **kw)


# iLQR options on the Cartpole: three regularisation levels in one batch (cartpole_levels), failed searches (cartpole_no_progress)
_row("levels_ls_0.3", "cartpole_levels", dict(line_search_decrease_factor=0.3))
_row("levels_ls_0.8", "cartpole_levels", dict(line_search_decrease_factor=0.8), shared=dict(iterations=8))
_row("levels_reg_factor", "cartpole_levels", dict(bp_reg_increase_factor=2.5))
_row("levels_reg_min", "cartpole_levels", dict(bp_reg_min=1e-2))
_row("levels_reg_initial", "cartpole_levels", dict(bp_reg_initial=0.05), late=True)
# (a loose cost tolerance in both runs, so that the gradient test is the one that decides whether a trajectory has converged)
_row("levels_gradient_tolerance", "cartpole_levels", dict(gradient_tolerance=0.1), shared=dict(cost_tolerance=1.0))
_row("no_progress_reg_fp_0.5", "cartpole_no_progress", dict(bp_reg_fp=0.5))
_row("no_progress_reg_fp_100", "cartpole_no_progress", dict(bp_reg_fp=100.0))
_row("no_progress_ls_0.8", "cartpole_no_progress", dict(line_search_decrease_factor=0.8))
# AL options on the small models
_row("al_penalty_max", "cartpole_al", dict(penalty_max=5.0))
_row("al_dual_max", "cartpole_al", dict(dual_max=2.0))
_row("al_clamps", "cartpole_al", dict(penalty_max=5.0, dual_max=2.0))
_row("al_penalty_initial", "cartpole_al", dict(penalty_initial=3.0), late=True)
_row("al_penalty_scaling", "cartpole_al", dict(penalty_scaling=3.0))
_row("al_cost_tolerance_intermediate", "cartpole_al", dict(cost_tolerance_intermediate=0.1))
_row("di2_penalty_max", "di2_levels", dict(penalty_max=5.0))
_row("di2_dual_max", "di2_levels", dict(dual_max=0.5))
_row("di2_iterations_total", "di2_levels", dict(iterations_total=7), late=True)
# ALTRO: the clamps in front of the polish, and the polish's own options
_row("altro_penalty_max", "di2_altro", dict(penalty_max=20.0))
_row("altro_dual_max", "di2_altro", dict(dual_max=1.0))
_row("altro_active_set_tolerance", "di2_altro", dict(active_set_tolerance_pn=0.5))
_row("altro_rho_primal", "di2_altro", dict(rho_primal=0.1))
# the polish alone on the batch of pn_cases that leaves a projection through the convergence-rate break: the threshold on the other
# side of the rate it measures there
_row("pn_r_threshold", PN.CASES["rate_and_linesearch"], dict(r_threshold=3.0))
# the Quadrotor (other translation units): iLQR options on the failing batches, AL options on the cone-constrained one
_row("quadrotor_ls_0.3", "quadrotor_w7", dict(line_search_decrease_factor=0.3))
# (three iterations: with five, 5 of the 40 trajectories amplify a last-bit change of the start beyond 1e-8)
_row("quadrotor_ls_0.8_deep", "quadrotor_w7", dict(line_search_decrease_factor=0.8), shared=dict(iterations=3))
_row("quadrotor_reg_factor", "quadrotor_w7", dict(bp_reg_increase_factor=2.5))
_row("quadrotor_reg_min", "quadrotor_w10", dict(bp_reg_min=1e-2))
_row("quadrotor_reg_initial", "quadrotor_w7", dict(bp_reg_initial=0.05))
_row("quadrotor_reg_fp", "quadrotor_w7", dict(bp_reg_fp=0.5), shared=WINDOW)
_row("quadrotor_gradient_tolerance", "quadrotor_w7", dict(gradient_tolerance=1.0), shared=dict(cost_tolerance=100.0, iterations=8))
_row("cone_clamps", QUADROTOR_CONE, dict(penalty_max=50.0, dual_max=0.05))
_row("cone_penalty_growth", QUADROTOR_CONE, dict(penalty_scaling=3.0, penalty_initial=5.0))
_row("cone_cost_tolerance_intermediate", QUADROTOR_CONE, dict(cost_tolerance_intermediate=10.0))
_row("cone_iterations_total", QUADROTOR_CONE, dict(iterations_total=7))

ILQR_SMALL = [n for n, r in ROWS.items() if r.solver == "ilqr" and not r.quadrotor]
ILQR_QUADROTOR = [n for n, r in ROWS.items() if r.solver == "ilqr" and r.quadrotor]
AL = [n for n, r in ROWS.items() if r.solver in ("al", "altro")]
# every option the rows must cover, on a small model / on the Quadrotor (the three polish options: small model only)
OPTIONS_ILQR = ("line_search_decrease_factor", "bp_reg_increase_factor", "bp_reg_min", "bp_reg_fp", "gradient_tolerance", "bp_reg_initial")
OPTIONS_AL = ("penalty_max", "dual_max", "penalty_initial", "penalty_scaling", "cost_tolerance_intermediate", "iterations_total")
OPTIONS_PN = ("active_set_tolerance_pn", "rho_primal", "r_threshold")
# calls of I.dual_update in the dual-update phases: enough for both clamps to bind (asserted by the CPU test)
DUAL_CALLS = 3
