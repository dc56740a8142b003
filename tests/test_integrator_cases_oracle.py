"""The rows of tests/integrator_cases.py vetted on the CPU oracle alone, and the oracle's own RK3 / Euler / RK4 steps held to the
longdouble restatement of integrator_cases (which goes through no solver code): what tests/test_gpu_integrators.py holds the kernels to.

Per row: every trajectory iterates at least three times, no integer of the solve changes when the start states move by the steps of
failure_cases.ULPS, the value mask of option_cases.stability leaves out at most a quarter of the batch, and the scheme changes the
solve (see integrator_cases.SAME_AS_RK4 for the three rows where it cannot); an ALTRO row hands the share of its batch that
integrator_cases.POLISHED states to the polish.  Run with ``-s`` for the per-row figures."""
import ctypes as C

import numpy as np
import pytest

import trajopt_amd as T
import failure_cases as F
import option_cases as O
import integrator_cases as IC

L = np.longdouble
PD = C.POINTER(C.c_double)


# ---------------------------------------------------------------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("name", list(IC.ROWS))
def test_row_is_a_sound_input(name, oracle):
    row, base = IC.ROWS[name], IC.BASE_OF[name]
    st, X, U = O.oracle_solve(row, oracle)[:3]
    B = X.shape[0]
    it = st["iterations"]
    mask, unstable = O.stability(row, oracle)
    X4 = O.oracle_solve(IC.RK4_ROWS[base], oracle)[1]
    diff = np.abs(X - X4).reshape(B, -1).max(axis=1)
    print(f"\n{name}: B = {B}, iterations {it.min()} .. {it.max()}, statuses {dict(zip(*np.unique(st['status'], return_counts=True)))}, "
          f"mask leaves out {int((~mask).sum())} of {B}, {int(unstable.sum())} unstable integers, "
          f"|X - X(RK4)| per trajectory {diff.min():.2e} .. {diff.max():.2e}")
    assert it.min() >= 3, f"{name}: a trajectory stops after {it.min()} iterations"
    assert not unstable.any(), f"{name}: integers of trajectories {np.where(unstable)[0]} change under last-bit changes of the start"
    assert 4 * int((~mask).sum()) <= B, f"{name}: the value mask leaves out {int((~mask).sum())} of {B} trajectories"
    if row.solver == "altro":
        share, polished = IC.POLISHED[base], int((st["iterations_pn"] >= 1).sum())
        print(f"{name}: {polished} of {B} trajectories projected, {st['iterations_pn'].max()} projections at most, c_max <= {st['c_max'].max():.1e}")
        assert (polished == 0) if share == 0 else (polished >= share * B), f"{name}: the polish projects {polished} of {B} trajectories"
    if name in IC.SAME_AS_RK4:
        # RK3 is exact on a double integrator under a held control, like RK4: the two runs agree to rounding (and say so, so that a
        # row that starts to differ is noticed)
        assert (F.trajectory_error(X, X4)[mask] <= 1e-8).all(), f"{name}: RK3 and RK4 differ on a double integrator"
    else:
        assert (diff > 1e-6).all(), f"{name}: trajectories {np.where(diff <= 1e-6)[0]} do not notice the integrator"


def test_rows_cover_both_schemes():
    for base, spec in IC._BASES.items():
        want = {"quadrotor_mrp_ilqr": {"rk3"}, "quadrotor_altro": {"rk3"}, "quadrotor_altro_unpolished": {"euler"}}.get(base, {"rk3", "euler"})
        assert {t for t in spec[4]} == want and all(f"{base}_{t}" in IC.ROWS for t in want)
    assert set(IC.PHASE_ONLY) == {"infeasible_cartpole", "hybrid", "vector_cartpole_mix"}


@pytest.mark.parametrize("which,scheme", IC.PHASE_ONLY_CASES, ids=[f"{w}_{IC.TAGS[s]}" for w, s in IC.PHASE_ONLY_CASES])
def test_phase_only_models_take_the_integrator(which, scheme, oracle):
    """The host mirror passes ``integration`` through for the three phase-only models: the handle is created, reports its scheme, and its
    rollout differs from the RK4 handle's wherever a nonlinear step is involved (the Cartpole steps of the infeasible problem and of
    the model vector; the hybrid double integrator's steps are exact under RK3 and RK4 and agree to rounding, under Euler they differ)."""
    p3, p4 = IC.PHASE_ONLY[which](oracle, scheme), IC.PHASE_ONLY[which](oracle, T.RK4)
    assert p3.integration == scheme and p3._desc.integrator == scheme
    if which == "infeasible_cartpole":
        # (the infeasible rollout reproduces the state guess whatever the scheme: the slack controls absorb the difference)
        d = np.abs(T.controls(p3) - T.controls(p4)).max()
        assert d > 1e-6
    else:
        T.rollout(p3); T.rollout(p4)
        d = np.abs(T.states(p3) - T.states(p4)).max()
        assert (d > 1e-6) if which == "vector_cartpole_mix" or scheme == T.Euler else (d <= 1e-12)
    print(f"\n{which}: {IC.TAGS[scheme]} against RK4 {d:.2e}")


# ------------------------------------------------------------------------------------ 2. one step of the oracle against the restatement
def _oracle_step(oracle, model, scheme, X, U, h):
    out = np.zeros_like(X)
    params = (C.c_double * 16)(*(list(model.params()) + [0.0] * 16)[:16])
    xn = np.zeros(model.n)
    for i in range(X.shape[0]):
        x, u = np.ascontiguousarray(X[i]), np.ascontiguousarray(U[i])
        oracle.call("discrete_dynamics", model.model_id, params, scheme, x.ctypes.data_as(PD), u.ctypes.data_as(PD), float(h), xn.ctypes.data_as(PD))
        out[i] = xn
    return out


def _step_inputs(model):
    rng = np.random.default_rng(23)
    K = 400
    if isinstance(model, T.Cartpole):
        X = np.c_[rng.uniform(-2, 2, K), rng.uniform(-2 * np.pi, 2 * np.pi, K), rng.uniform(-5, 5, K), rng.uniform(-40, 40, K)]
        X[:8, 3] = [40.0, -40.0, 39.5, -39.5, 0.0, 1e-3, 15.0, -15.0]
        return X, rng.uniform(-10, 10, (K, 1))
    return rng.uniform(-5, 5, (K, model.n)), rng.uniform(-10, 10, (K, model.m))


@pytest.mark.parametrize("model", [T.Cartpole(), T.DoubleIntegrator(0.8, 2), T.DoubleIntegrator(0.8, 3)], ids=["cartpole", "di2", "di3"])
def test_one_step_of_the_oracle_against_the_restatement(model, oracle):
    """discrete_dynamics of the oracle against the longdouble restatement, 400 states (Cartpole: |thetadot| up to 40 rad/s) x h in
    (0.05, 0.1), error per state relative to max(1, |x+|).  RK4 is measured first — it is the scheme the reference goldens pin hardest —
    and RK3 and Euler are allowed four times the largest RK4 deviation on the same inputs (rounding of the same number of stages or
    fewer, with a margin for the different stage points).
    Measured RK4 deviation: Cartpole 2.77e-16 (RK3 3.26e-16, Euler 2.37e-16 against the 1.11e-15 allowed), 2-D double integrator
    1.99e-16 (RK3 1.99e-16, Euler 1.11e-16), 3-D double integrator 1.64e-16 (RK3 1.64e-16, Euler 1.30e-16)."""
    f = IC.cartpole_f if isinstance(model, T.Cartpole) else IC.double_integrator_f(model.mass, model.D)
    X, U = _step_inputs(model)
    dev = {}
    for scheme in (T.RK4, T.RK3, T.Euler):
        worst = 0.0
        for h in (0.05, 0.1):
            want = IC.step(f, scheme, X, U, h)
            got = _oracle_step(oracle, model, scheme, X, U, h)
            err = np.abs(got.astype(L) - want).max(axis=1) / np.maximum(1.0, np.abs(want).max(axis=1))
            worst = max(worst, float(err.max()))
        dev[scheme] = worst
    print(f"\none step, {type(model).__name__} n = {model.n}: RK4 deviation {dev[T.RK4]:.3e} -> RK3 / Euler allowed {4 * dev[T.RK4]:.3e}; "
          f"RK3 {dev[T.RK3]:.3e}, Euler {dev[T.Euler]:.3e}")
    assert 0 < dev[T.RK4] <= 1e-14, "the RK4 step itself is off: 1e-14 is ~50 ulp of a result of magnitude 1"
    assert dev[T.RK3] <= 4 * dev[T.RK4] and dev[T.Euler] <= 4 * dev[T.RK4]


# ------------------------------------------------------------------------------------------------------------ 3. order of convergence
ORDER = {T.Euler: 1, T.RK3: 3, T.RK4: 4}
ORDER_H = {T.Euler: 1.0 / 256, T.RK3: 1.0 / 16, T.RK4: 1.0 / 64}     # the restatement alone is within 0.15 of the order at these (asserted)
_X0, _U = np.array([0.1, 0.4, -0.2, 0.3]), np.array([0.7])


def _terminal(stepper, h):
    n = int(round(1.0 / h))
    x = _X0.copy()
    for _ in range(n):
        x = stepper(x, h)
    return np.asarray(x, L)


def test_order_of_convergence(oracle):
    """Terminal state of a 1 s Cartpole rollout under a constant control, step sizes h, h/2, h/4, error against the restatement's RK4 at
    h/64: the observed order log2(e(h) / e(h/2)) is within 0.15 of 1 / 3 / 4 for the restatement and within 0.3 for the
    oracle.  No solver code is involved."""
    model = T.Cartpole()
    for scheme, order in ORDER.items():
        h0 = ORDER_H[scheme]
        ref = _terminal(lambda x, h: IC.step(IC.cartpole_f, T.RK4, x, _U, h), h0 / 64)
        for who, tol in (("restatement", 0.15), ("oracle", 0.3)):
            if who == "restatement":
                stepper = lambda x, h: IC.step(IC.cartpole_f, scheme, x, _U, h)
            else:
                stepper = lambda x, h: _oracle_step(oracle, model, scheme, np.asarray(x, np.float64)[None], _U[None], h)[0]
            e = [float(np.abs(_terminal(stepper, h) - ref).max()) for h in (h0, h0 / 2, h0 / 4)]
            got = [np.log2(e[0] / e[1]), np.log2(e[1] / e[2])]
            print(f"\norder of {IC.TAGS[scheme]} ({who}), h = {h0}: errors {e[0]:.3e} {e[1]:.3e} {e[2]:.3e}, observed {got[0]:.3f} {got[1]:.3f}")
            assert all(abs(g - order) <= tol for g in got), f"{IC.TAGS[scheme]} ({who}): observed order {got}, expected {order}"


# ------------------------------------------------------------------------------------------------ 4. the angle-addition batch
@pytest.mark.parametrize("scheme", [T.RK4, T.RK3, T.Euler], ids=["rk4", "rk3", "euler"])
def test_threshold_batch_straddles_the_threshold(scheme, oracle):
    """The batch of test_gpu_integrators.test_angle_addition_threshold, by the restatement: every later stage of every step of wave 0 stays
    below 0.6, the largest stage of every step of wave 2 lies above 0.75, wave 1 alternates lane by lane on its first step with four lanes
    within 1e-3 of the threshold on each side — and the oracle's rollout of it meets the restatement at rtol 1e-10 / atol 1e-12."""
    x0, U = IC.threshold_batch(scheme)
    d = IC.threshold_deltas(scheme, x0, U)
    assert x0.shape == (192, 4) and np.isfinite(x0).all() and np.abs(x0).max() < 50
    assert (d[:64] < 0.6).all() and (d[128:] > IC.TRIG_SMALL_MAX).all()
    first = np.asarray(d[64:128, 0], np.float64)
    assert (first[0::2] < IC.TRIG_SMALL_MAX).all() and (first[1::2] > IC.TRIG_SMALL_MAX).all()
    near = np.abs(first - IC.TRIG_SMALL_MAX) < IC.NEAR
    assert (near & (first < IC.TRIG_SMALL_MAX)).sum() == 4 and (near & (first > IC.TRIG_SMALL_MAX)).sum() == 4
    p = IC.threshold_problem(oracle, scheme, x0, U)
    T.rollout(p)
    X = T.states(p)
    assert np.abs(X).max() < 100
    np.testing.assert_allclose(X, IC.rollout(IC.cartpole_f, scheme, x0, U, IC.THRESHOLD_DT).astype(np.float64), rtol=1e-10, atol=1e-12)
    print(f"\nthreshold batch {IC.TAGS[scheme]}: wave 0 below {float(d[:64].max()):.3f}, wave 2 above {float(d[128:].min()):.3f}, "
          f"nearest lanes {np.sort(np.abs(first - IC.TRIG_SMALL_MAX))[:8]}")
