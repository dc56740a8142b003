"""Batches that go badly: problems whose trajectories restart the backward pass at different regularisation levels, run into
bp_reg_max, fail their line search, or end a solve as MAXIMUM_COST / NO_PROGRESS / REGULARIZATION_MAX — several such classes inside
one batch, over both 64-lane tiles and a ragged last one.  Negative entries in an LQRObjective / QuatLQRCost weight vector are
accepted by both libraries and make Quu indefinite; per-trajectory initial controls spread the batch over the classes.

Shared by tests/test_failure_cases_oracle.py (which vets every case on the CPU oracle alone: class mix, decision margins, stability
of every integer under last-bit changes of the inputs) and tests/test_gpu_failure_paths.py (which runs them on the GPU kernels).
No GPU is needed to import this module."""
import math

import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

S = T.capi
# the perturbed runs of the stability checks: start states moved by this many ulp.  Both signs of each size, because a trajectory can
# be sensitive to one and not the other: the oracle's solution of cartpole_levels, trajectory 37, moves by 1.3e-7 under -2 ulp and by
# 3e-10 under +2
ULPS = (1, -1, 2, -2, 3, -3, 8, -8)


def shift_ulp(x, k):
    """Every entry of x moved by k representable numbers (k < 0: towards -inf)."""
    x = np.array(x, dtype=np.float64)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


class Case:
    """One failing batch.  ``build(lib, ulp)`` creates the problem (every solver option is a creation option, so the phase API
    and the solves see the same ones); ``solver``: "ilqr" | "al" | "altro"; ``expect``: the class labels (see classify) the
    case is meant to exercise; ``statuses``: the terminal statuses a solve must show; ``small``: a model small enough for the
    float128 restatement of the backward pass (every model but the Quadrotor)."""

    def __init__(self, name, build, solver, expect, statuses, small=True):
        self.name, self._build, self.solver, self.expect, self.statuses, self.small = name, build, solver, expect, statuses, small

    def build(self, lib, ulp=0, **opts):
        """-> the problem; ``p.case_options`` holds the SolverOptions it was created with."""
        p = self._build(lib, opts)
        if ulp:
            p.set_initial_state(shift_ulp(p.x0, ulp))
        return p

    def solve(self, lib, ulp=0, **opts):
        """-> (stats dict of copies + total_iterations, X, U, prob)"""
        p = self.build(lib, ulp, **opts)
        Solver = {"ilqr": T.iLQRSolver, "al": T.ALSolver, "altro": T.ALTROSolver}[self.solver]
        s = Solver(p).solve()
        st = {k: np.array(v).copy() for k, v in s.stats.items()}
        st["total_iterations"] = int(s.total_iterations)
        return st, T.states(p), T.controls(p), p

    def first_pass(self, lib, ulp=0, forward=True, **opts):
        """rollout / expand / backwardpass / gains / forwardpass through the phase API."""
        p = self.build(lib, ulp, **opts)
        T.rollout(p)
        I.expand(p)
        I.backwardpass(p)
        g = I.gains(p)
        out = dict(prob=p, gains=g, rho=g["rho"].copy(), bpfail=g["rho"] > p.case_options.bp_reg_max)
        if forward:
            ls, J = I.forwardpass(p)
            out.update(ls=ls, J=J, X=T.states(p), U=T.controls(p), rho_after=I.gains(p)["rho"])
        return out


def _options(lib, base, extra):
    kw = dict(base)
    kw.update(extra)
    return T.SolverOptions(lib=lib, **kw)


def _spread(B):
    """Amplitudes in [0, 1) scattered over the batch (b -> 29 b mod B, a permutation for the batch sizes used here), so that the
    few trajectories of a ragged last tile cover small and large ones like the full tile does."""
    assert math.gcd(29, B) == 1
    return ((29 * np.arange(B)) % B) / B


def _cartpole(B=70, N=41, tf=2.0, Qf=(100.0, 100.0, 100.0, 100.0), constrained=False, u_bnd=3.0, amp=2.0, **base):
    def build(lib, extra):
        model = T.Cartpole()
        n, m = model.dims()
        xf = np.array([0.0, math.pi, 0.0, 0.0])
        obj = T.LQRObjective(np.full(n, 1e-2), np.full(m, 1e-1), np.array(Qf, dtype=np.float64), xf, N, checks=False)
        cons = T.ConstraintList(n, m, N)
        if constrained:
            T.add_constraint(cons, T.BoundConstraint(n, m, u_min=-u_bnd, u_max=u_bnd), range(1, N))
            T.add_constraint(cons, T.GoalConstraint(xf), N)
        o = _options(lib, base, extra)
        p = T.Problem(model, obj, np.zeros(n), tf, xf=xf, constraints=cons, batch=B, lib=lib, options=o)
        p.case_options = o
        p.set_initial_state(configs.cartpole_x0(B, 0))
        b, k = np.arange(B)[:, None], np.arange(N - 1)[None, :]
        T.initial_controls(p, (amp * _spread(B)[:, None] * np.sin(0.3 * k + 0.1 * b))[:, :, None])
        return p
    return build


def _double_integrator(B=70, N=21, tf=2.0, R=(0.1, 0.1), Qf=(10.0, 10.0, 10.0, 10.0), u_bnd=None, amp=1.0, integration=T.RK4, **base):
    """2-D double integrator (m = 2).  A linear model with a quadratic cost has the same Quu for every trajectory; the control bounds
    bring the trajectories apart: every violated bound adds its penalty to Quu's diagonal, knot by knot."""
    def build(lib, extra):
        model = T.DoubleIntegrator(0.8, 2)
        n, m = model.dims()
        xf = np.array([1.0, -2.0, 0.0, 0.0])
        obj = T.LQRObjective(np.ones(n), np.array(R, dtype=np.float64), np.array(Qf, dtype=np.float64), xf, N, checks=False)
        cons = T.ConstraintList(n, m, N)
        if u_bnd is not None:
            T.add_constraint(cons, T.BoundConstraint(n, m, u_min=-u_bnd, u_max=u_bnd), range(1, N))
            T.add_constraint(cons, T.GoalConstraint(xf), N)
        o = _options(lib, base, extra)
        p = T.Problem(model, obj, np.zeros(n), tf, xf=xf, constraints=cons, batch=B, lib=lib, options=o, integration=integration)
        p.case_options = o
        p.set_initial_state(np.linspace(-0.5, 0.5, B)[(17 * np.arange(B)) % B][:, None] * np.ones((B, n)))   # (scattered like the amplitudes, not with them)
        b, k = np.arange(B)[:, None, None], np.arange(N - 1)[None, :, None]
        j = np.arange(m)[None, None, :]
        T.initial_controls(p, amp * _spread(B)[:, None, None] * np.sin(0.3 * k + 0.1 * b + 1.3 * j))
        return p
    return build


def _quadrotor(B=40, N=41, tf=1.0, neg_index=10, neg_value=-5.0, **base):
    def build(lib, extra):
        model = T.Quadrotor()
        n, m = model.dims()
        th = math.radians(135.0) / 2
        xf = np.zeros(n); xf[:3] = [2.0, 3.0, 1.0]; xf[3:7] = [math.cos(th), 0.0, 0.0, math.sin(th)]
        Qd = np.array([1.0, 1, 1, 0, 0, 0, 0, .1, .1, .1, .1, .1, .1])
        Rd = np.full(m, 1e-2)
        Qf = 100.0 * Qd
        Qf[neg_index] = neg_value
        uh = model.hover_control()
        obj = T.Objective(T.QuatLQRCost(Qd, Rd, xf, uh, w=1.0), T.QuatLQRCost(Qf, Rd, xf, uh, w=1.0, terminal=True), N)
        o = _options(lib, base, extra)
        p = T.Problem(model, obj, np.zeros(n), tf, xf=xf, constraints=T.ConstraintList(n, m, N), batch=B, lib=lib, options=o)
        p.case_options = o
        p.set_initial_state(configs.quadrotor_x0(B, 0))
        z = np.random.default_rng(7).standard_normal((B, N - 1, m))
        T.initial_controls(p, uh + 0.5 * _spread(B)[:, None, None] * z)
        return p
    return build


def classify(case, lib):
    """-> (labels, info): labels[b] is the set of classes trajectory b falls into —
    "rho=<value>" (the regularisation its FIRST backward pass left; "rho=0.000000": no restart), "bpfail" (that pass ran into
    bp_reg_max), "ls_fail" (its first line search failed), "status=<n>" (how its solve ended)."""
    fp = case.first_pass(lib)
    st, X, U, p = case.solve(lib)
    labels = []
    for b in range(p.B):
        L = set()
        if fp["bpfail"][b]:
            L.add("bpfail")
        else:
            L.add(f"rho={fp['rho'][b]:.6f}")
            if fp["ls"][b] < 0:
                L.add("ls_fail")
        L.add(f"status={int(st['status'][b])}")
        labels.append(L)
    return labels, dict(first=fp, stats=st, X=X, U=U)


def histogram(labels):
    h = {}
    for L in labels:
        for c in L:
            h[c] = h.get(c, 0) + 1
    return dict(sorted(h.items()))


def trajectory_error(A, R):
    """The relative measure of test_gpu_parity.assert_trajectories_close: max |A - R| / max(1, max |R|) per trajectory."""
    B = R.shape[0]
    return np.abs(A - R).reshape(B, -1).max(axis=1) / np.maximum(1.0, np.abs(R).reshape(B, -1).max(axis=1))


def trajectories_close(A, R, rtol):
    return trajectory_error(A, R) <= rtol


_masks = {}


def value_mask(case, oracle):
    """The trajectories of a short solve whose VALUES mean something: X, U and J agree to 1e-8 between the oracle's base run and each
    of its runs from start states moved by the steps of ULPS.  The others amplify a last-bit difference of the inputs beyond any
    tolerance a second implementation could be held to (their integers are still compared).  Computed on the oracle alone, once per
    case."""
    if case.name not in _masks:
        st, X, U, _ = case.solve(oracle)
        ok = np.ones(X.shape[0], bool)
        for ulp in ULPS:
            s2, X2, U2, _ = case.solve(oracle, ulp=ulp)
            ok &= trajectories_close(X2, X, 1e-8) & trajectories_close(U2, U, 1e-8)
            ok &= np.abs(s2["cost"] - st["cost"]) <= 1e-8 * np.maximum(1.0, np.abs(st["cost"]))
        _masks[case.name] = ok
    return _masks[case.name]


# ---------------------------------------------------------------------------------------------------------------- float128 Riccati
def riccati_with_restarts(A, Bm, E, rho, drho, opts):
    """The backward recursion with its restart rule for ONE trajectory, restated in numpy's extended precision (np.longdouble):
    A [N-1, ne, ne], Bm [N-1, ne, m], E = the trajectory's slice of I.cost_expansion.  The regularisation schedule itself is
    float64 arithmetic (it has to reproduce rho exactly).  -> dict(K, d, dV, rho (after the pass), drho, failed, rhos (every level
    tried), pivots (every Cholesky pivot tested: (value, scale, accepted), scale = the largest sum of magnitudes |cost Quu_ii| +
    |(B'SB)_ii| + rho over the diagonal — at least the largest diagonal entry of Quu + rho I))."""
    L = np.longdouble
    f, rmin, rmax = float(opts.bp_reg_increase_factor), float(opts.bp_reg_min), float(opts.bp_reg_max)
    A, Bm = A.astype(L), Bm.astype(L)
    Qxx, Quu, Qux, qx, qu = (E[k].astype(L) for k in ("Qxx", "Quu", "Qux", "qx", "qu"))
    N, m = Qxx.shape[0], Quu.shape[1]
    K, d = np.zeros((N - 1, m, A.shape[1]), L), np.zeros((N - 1, m), L)
    rho, drho = float(rho), float(drho)
    rhos, pivots, failed = [rho], [], False
    while True:
        restart = False
        Sm, s = Qxx[N - 1].copy(), qx[N - 1].copy()
        dV = [L(0), L(0)]
        for k in range(N - 2, -1, -1):
            SA, SB = Sm @ A[k], Sm @ Bm[k]
            Gx, Gu = qx[k] + A[k].T @ s, qu[k] + Bm[k].T @ s
            Gxx, BSB, Gux = Qxx[k] + A[k].T @ SA, Bm[k].T @ SB, Qux[k] + Bm[k].T @ SA
            Guu = Quu[k] + BSB
            M = Guu + L(rho) * np.eye(m, dtype=L)
            scale = float(np.max(np.abs(np.diag(Quu[k])) + np.abs(np.diag(BSB)) + L(rho)))
            C = np.zeros((m, m), L)
            ok = True
            for j in range(m):   # lower Cholesky, pivot by pivot
                sj = M[j, j] - C[j, :j] @ C[j, :j]
                ok = bool(sj > 0)
                pivots.append((float(sj), scale, ok))
                if not ok:
                    break
                C[j, j] = np.sqrt(sj)
                for i in range(j + 1, m):
                    C[i, j] = (M[i, j] - C[i, :j] @ C[j, :j]) / C[j, j]
            if not ok:
                drho = max(drho * f, f)
                rho = max(rho * drho, rmin)
                rhos.append(rho)
                if rho > rmax:
                    failed = True
                else:
                    restart = True
                break
            Mi = np.linalg.inv(M.astype(np.float64)).astype(L)
            Mi = Mi @ (2 * np.eye(m, dtype=L) - M @ Mi)   # one Newton step: the inverse to extended precision
            Mi = Mi @ (2 * np.eye(m, dtype=L) - M @ Mi)
            K[k], d[k] = -Mi @ Gux, -Mi @ Gu
            s = Gx + K[k].T @ (Guu @ d[k]) + K[k].T @ Gu + Gux.T @ d[k]
            Sn = Gxx + K[k].T @ Guu @ K[k] + K[k].T @ Gux + Gux.T @ K[k]
            Sm = 0.5 * (Sn + Sn.T)
            dV[0] += d[k] @ Gu
            dV[1] += 0.5 * (d[k] @ (Guu @ d[k]))
        if failed or not restart:
            break
    if not failed:
        drho = min(drho / f, 1.0 / f)
        r = rho * drho
        rho = r if r > rmin else 0.0
    return dict(K=K.astype(np.float64), d=d.astype(np.float64), dV=np.array([float(dV[0]), float(dV[1])]), rho=rho, drho=drho,
                failed=failed, rhos=rhos, pivots=pivots)


# ------------------------------------------------------------------------------------------------------------------------ the cases
CASES = {}


def _add(case):
    CASES[case.name] = case
    return case


_NEG = (100.0, 100.0, 100.0, -1.0)      # the pole's angular velocity is REWARDED at the terminal knot: Quu = R + B'SB goes indefinite

# three regularisation levels in one batch (none / one restart round / several); the same with bp_reg_max between the second and the
# third level, so that the third class fails its backward pass and the solve shows REGULARIZATION_MAX next to MAX_ITERATIONS
_add(Case("cartpole_levels", _cartpole(Qf=_NEG, amp=4.0, iterations=12), "ilqr",
          expect=["rho=0.000000", "rho=0.087112", "rho=5.986311"], statuses=[S.MAX_ITERATIONS]))
_add(Case("cartpole_regmax", _cartpole(Qf=_NEG, amp=4.0, iterations=12, bp_reg_max=1.0), "ilqr",
          expect=["rho=0.000000", "rho=0.087112", "bpfail", "status=10", "status=3"], statuses=[S.REGULARIZATION_MAX, S.MAX_ITERATIONS]))
_add(Case("cartpole_max_cost", _cartpole(amp=4.0, iterations=12, max_cost_value=400.0), "ilqr",
          expect=["status=5", "status=3"], statuses=[S.MAXIMUM_COST, S.MAX_ITERATIONS]))
# a line search of two step sizes with a narrow acceptance window: failed searches from the first pass on; part of the batch stalls
# (NO_PROGRESS after dJ_counter_limit failures in a row), part goes on to the iteration limit
_add(Case("cartpole_no_progress", _cartpole(amp=4.0, iterations=12, iterations_linesearch=2, line_search_lower_bound=0.3,
                                            line_search_upper_bound=0.95, dJ_counter_limit=2), "ilqr",
          expect=["ls_fail", "status=8", "status=3"], statuses=[S.NO_PROGRESS, S.MAX_ITERATIONS]))
# AL: the goal constraint's penalty adds to the terminal weights, so the negative one is stronger; an inner REGULARIZATION_MAX /
# MAXIMUM_COST ends the AL solve, the rest runs out of outer iterations
_add(Case("cartpole_al", _cartpole(Qf=(100.0, 100.0, 100.0, -2.0), amp=6.0, constrained=True, bp_reg_max=1.0, max_cost_value=600.0,
                                   iterations=4, iterations_outer=3), "al",
          expect=["rho=0.000000", "rho=0.087112", "bpfail", "status=10", "status=5", "status=4"],
          statuses=[S.REGULARIZATION_MAX, S.MAXIMUM_COST, S.MAX_ITERATIONS_OUTER]))
# m = 2: a negative control weight; the active control bounds (penalty on Quu's diagonal, knot by knot) bring the batch apart
_add(Case("di2_levels", _double_integrator(R=(0.1, -0.09), u_bnd=0.2, amp=4.0, iterations=4, iterations_outer=3), "al",
          expect=["rho=0.000000", "rho=0.087112", "rho=5.986311"], statuses=[S.MAX_ITERATIONS_OUTER]))
_add(Case("di2_regmax", _double_integrator(R=(0.1, -0.09), u_bnd=0.2, amp=4.0, iterations=4, iterations_outer=3, bp_reg_max=1.0), "al",
          expect=["rho=0.000000", "rho=0.087112", "bpfail", "status=10"], statuses=[S.REGULARIZATION_MAX]))
_add(Case("quadrotor_w10", _quadrotor(neg_index=10, neg_value=-5.0, iterations=5), "ilqr", small=False,
          expect=["rho=658.201823", "rho=115792.089237"], statuses=[S.MAX_ITERATIONS]))
_add(Case("quadrotor_w7", _quadrotor(neg_index=7, neg_value=-1.0, iterations=5), "ilqr", small=False,
          expect=["rho=0.000000", "rho=0.087112"], statuses=[S.MAX_ITERATIONS]))
# ALTRO on the convex double integrator: the penalties of the trajectories that cannot meet bounds and goal together push the AL cost
# over max_cost_value (MAXIMUM_COST ends their AL stage, the polish leaves them alone), a few run out of outer iterations, the rest
# converge and are polished
_add(Case("di2_altro", _double_integrator(R=(0.1, 0.1), u_bnd=2.0, amp=4.0, max_cost_value=300.0), "altro",
          expect=["status=5", "status=4", "status=2"], statuses=[S.MAXIMUM_COST, S.MAX_ITERATIONS_OUTER, S.SOLVE_SUCCEEDED]))
# unconstrained and linear: every trajectory has the same Quu, so the whole batch restarts alike — the one m = 2 problem the scan
# kernel (unconstrained problems only) can be given
_add(Case("di2_uniform", _double_integrator(R=(0.1, -0.09), amp=4.0, iterations=4), "ilqr",
          expect=["rho=5.986311"], statuses=[S.MAX_ITERATIONS]))
# the Quadrotor with bp_reg_max between its two levels
_add(Case("quadrotor_regmax", _quadrotor(neg_index=10, neg_value=-5.0, iterations=5, bp_reg_max=1e4), "ilqr", small=False,
          expect=["rho=658.201823", "bpfail", "status=10", "status=3"], statuses=[S.REGULARIZATION_MAX, S.MAX_ITERATIONS]))
