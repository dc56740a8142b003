"""to_policy_rollout on the MI355X: S perturbed samples per solved trajectory under the feedback law u = ū_k + α d_k + K_k (x ⊖ x̄_k).

Expected values come from a CPU restatement of the operator (``restate``, tests/policy_ref.py) in the order the header gives: it steps with the oracle's
``discrete_dynamics`` and ``state_diff`` and takes the nominal trajectory and the gains FROM THE HIP HANDLE (T.states, T.controls,
I.gains), so only the new kernel is under test.  J and c_max come from the oracle itself: a sample's closed-loop (X, U) is loaded into
an oracle problem (initial_states / initial_controls) and evaluated with T.cost / T.max_violation.

Tolerance 1e-9 (relative, max norm per sample): open-loop rollouts are held to 1e-11 (test_gpu_parity.py::test_rollout_and_cost) and the
closed loop amplifies a 1e-9 relative disturbance of K at most 112-fold at these shapes, so rounding stays orders of magnitude below.

Every comparison prints its largest deviation (``policy_rollout deviation ...``, visible with ``-s``).  OBSERVED on an MI355X: not recorded
yet — this file has not run on a GPU; the figures belong here once it has, with an explanation for any above 1e-11.
"""
import ctypes as C

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

import policy_ref
from policy_ref import RTOL, Stepper, compare, ref_slice, restate, sample_starts   # (the restatement: shared with tests/test_policy_host.py)

pytestmark = pytest.mark.gpu

S_MAX = 70
S_VALUES = [1, 3, 64, 70]   # 1, 3: packed lane map; 64: one full uniform wave; 70: a second wave with 6 live lanes


# ------------------------------------------------------------------------------------------------ cases
def _hybrid(lib, batch):
    from test_hybrid_dims import hybrid_problem
    return hybrid_problem(lib, batch=batch)[0]


def _quickstart(lib, batch):
    p = configs.quickstart_problem(batch=batch, lib=lib)
    x0 = np.tile(np.array([0.2, 0.1, 0.0, 0.0]), (batch, 1))
    x0[1::2, 0] = -0.2
    p.set_initial_state(x0)
    return p


CASES = {
    "cartpole5": dict(build=lambda lib, batch: configs.cartpole_problem(batch=batch, N=31, tf=3.0, lib=lib), B=5, solver=T.iLQRSolver, sigma=0.05),
    "cartpole70": dict(build=lambda lib, batch: configs.cartpole_problem(batch=batch, N=31, tf=3.0, lib=lib), B=70, solver=T.iLQRSolver, sigma=0.05),
    "quadrotor": dict(build=lambda lib, batch: configs.quadrotor_problem(batch=batch, N=21, tf=1.0, lib=lib), B=3, solver=T.iLQRSolver, sigma=0.01),
    "quickstart": dict(build=_quickstart, B=3, solver=T.ALSolver, sigma=0.05),
    "hybrid": dict(build=_hybrid, B=3, solver=T.iLQRSolver, sigma=0.05),
}


def oracle_cost_and_violation(oracle, case, X, U):
    """J and c_max of every closed-loop sample from the oracle: the samples loaded as the trajectories of one oracle problem."""
    return policy_ref.oracle_cost_and_violation(oracle, CASES[case]["build"], X, U)


_cache = {}


def solved(case, hip, oracle):
    """The case's problem solved once on the GPU, its nominal and gains, S_MAX start states and the restatement for them (alpha = 0, no
    clamp, the planning model as the plant); the S < S_MAX runs use the first S samples, which share the reference."""
    if case not in _cache:
        c = CASES[case]
        p = c["build"](hip, c["B"])
        c["solver"](p).solve()
        I.expand(p); I.backwardpass(p)
        g = I.gains(p)
        Xbar, Ubar = T.states(p), T.controls(p)
        X0s = sample_starts(p, Xbar, c["sigma"], S_MAX)
        Xr, Ur, dxr = restate(oracle, p, Xbar, Ubar, g["K"], g["d"], X0s)
        Jr, cr = oracle_cost_and_violation(oracle, case, Xr, Ur)
        _cache[case] = dict(p=p, Xbar=Xbar, Ubar=Ubar, K=g["K"], d=g["d"], X0s=X0s, ref=(Xr, Ur, dxr, Jr, cr))
    return _cache[case]


# ------------------------------------------------------------------------------------------------ 1. parity with the restatement
@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_restatement(case, S, hip, oracle):
    c = solved(case, hip, oracle)
    r = T.policy_rollout(c["p"], c["X0s"][:, :S], trajectories=True)
    compare(f"{case} S={S}", r, ref_slice(c["ref"], S))
    s_only = T.policy_rollout(c["p"], c["X0s"][:, :S])          # the summary-only call (no staging) gives the same numbers
    assert s_only.X is None and s_only.U is None
    for k in ("J", "c_max", "dx_max", "status", "k_limit"):
        np.testing.assert_array_equal(getattr(s_only, k), getattr(r, k), err_msg=k)


def test_chunked_trajectory_download_equals_one_chunk(hip, oracle, monkeypatch):
    """X / U leave the device through a bounded staging pair, one chunk of waves at a time: one wave per chunk gives the same arrays."""
    c = solved("cartpole70", hip, oracle)
    for S in (3, 70):
        whole = T.policy_rollout(c["p"], c["X0s"][:, :S], trajectories=True)
        monkeypatch.setenv("TRAJOPT_POLICY_CHUNK_WAVES", "1")
        parts = T.policy_rollout(c["p"], c["X0s"][:, :S], trajectories=True)
        monkeypatch.delenv("TRAJOPT_POLICY_CHUNK_WAVES")
        for k in ("X", "U", "J", "c_max", "dx_max", "status", "k_limit"):
            np.testing.assert_array_equal(getattr(parts, k), getattr(whole, k), err_msg=f"S={S} {k}")


def test_lane_maps_agree(hip, oracle, monkeypatch):
    """The packed (per-lane pointers) and the uniform (scalar fetch) lane maps run the same body: at S = 64, where either can serve, both
    meet the restatement."""
    for case in ("cartpole5", "quadrotor"):
        c = solved(case, hip, oracle)
        monkeypatch.setenv("TRAJOPT_POLICY_MAP", "packed")
        r = T.policy_rollout(c["p"], c["X0s"][:, :64], trajectories=True)
        monkeypatch.delenv("TRAJOPT_POLICY_MAP")
        compare(f"{case} S=64 packed", r, ref_slice(c["ref"], 64))


# ------------------------------------------------------------------------------------------------ 2. nominal sample
@pytest.mark.parametrize("case", ["cartpole5", "quadrotor", "hybrid"])
def test_nominal_sample_is_the_open_loop_rollout(case, hip, oracle):
    """Sample 0 starts at x0 with alpha = 0: dx stays 0, so the closed loop applies the nominal controls and must land on T.rollout's states."""
    c = solved(case, hip, oracle)
    p = c["p"]
    r = T.policy_rollout(p, c["X0s"][:, :1], trajectories=True)
    T.rollout(p)                                      # the nominal of a solve is a rollout of its controls already; re-rolled for the comparison
    Xn = T.states(p)
    np.testing.assert_allclose(r.X[:, 0], Xn, rtol=1e-12, atol=1e-12)
    assert r.dx_max.max() <= 1e-12
    np.testing.assert_allclose(Xn, c["Xbar"], rtol=1e-12, atol=1e-12)
    T.initial_states(p, c["Xbar"])                    # the shared handle keeps the nominal the reference was computed for


# ------------------------------------------------------------------------------------------------ 3. the shipped forward pass
@pytest.mark.parametrize("build", [lambda hip: configs.cartpole_problem(batch=9, N=31, tf=3.0, lib=hip),
                                   lambda hip: configs.quadrotor_problem(batch=5, N=21, tf=1.0, lib=hip)], ids=["cartpole", "quadrotor"])
def test_reproduces_the_accepted_step_of_the_forward_pass(build, hip):
    """With alpha = 0.5^ls and the gains of the backward pass, one sample from x0 IS the line-search candidate the forward pass accepts."""
    p = build(hip)
    T.rollout(p)
    J0 = T.cost(p)
    I.expand(p); I.backwardpass(p)
    x0s = np.ascontiguousarray(T.states(p)[:, None, 0, :])
    tries = [T.policy_rollout(p, x0s, alpha=0.5 ** i, refresh_gains=False, trajectories=True) for i in range(8)]   # before the forward pass
    ls, Jn = I.forwardpass(p)
    Xa, Ua = T.states(p), T.controls(p)
    checked = 0
    for b in range(p.B):
        if ls[b] < 0 or ls[b] >= len(tries) or Jn[b] == J0[b]:
            continue
        r = tries[ls[b]]
        np.testing.assert_allclose(r.X[b, 0], Xa[b], rtol=1e-11, atol=1e-11, err_msg=f"trajectory {b}, ls {ls[b]}")
        np.testing.assert_allclose(r.U[b, 0], Ua[b], rtol=1e-11, atol=1e-11, err_msg=f"trajectory {b}, ls {ls[b]}")
        np.testing.assert_allclose(r.J[b, 0], Jn[b], rtol=1e-11)
        checked += 1
    print(f"forward-pass cross-check: {checked} of {p.B} trajectories compared, ls = {list(ls)}")
    assert checked >= 1, (ls, checked)


# ------------------------------------------------------------------------------------------------ 4. saturation, plant mismatch
def test_saturation(hip, oracle):
    """Controls clamped to [-3, 3].  The start states are spread with sigma = 0.2 here: at the 0.05 of the parity test the unclamped law
    never asks for more than |u| = 2.45 on this problem (restatement on the CPU, seeds 0 .. 11, 210 samples each; the nominal peaks at
    1.92), so the clamp would not engage; at 0.2 it does for 14 of the 210 samples (the unclamped law asks for up to 3.6)."""
    c = solved("quickstart", hip, oracle)
    p, S = c["p"], 70
    X0s = sample_starts(p, c["Xbar"], 0.2, S)
    Xr, Ur, dxr = restate(oracle, p, c["Xbar"], c["Ubar"], c["K"], c["d"], X0s, u_min=np.full(p.m, -3.0), u_max=np.full(p.m, 3.0))
    assert np.abs(Ur).max() == 3.0, "the clamp must be active in the reference"
    Jr, cr = oracle_cost_and_violation(oracle, "quickstart", Xr, Ur)
    r = T.policy_rollout(p, X0s, u_min=-3.0, u_max=3.0, trajectories=True)
    compare("quickstart clamp S=70", r, (Xr, Ur, dxr, Jr, cr))
    assert np.abs(r.U).max() == 3.0
    r3 = T.policy_rollout(p, X0s[:, :3], u_min=[-3.0, -3.0], u_max=[3.0, 3.0], trajectories=True)
    compare("quickstart clamp S=3", r3, ref_slice((Xr, Ur, dxr, Jr, cr), 3))


def test_plant_mismatch(hip, oracle):
    c = solved("cartpole5", hip, oracle)
    p, S = c["p"], 70
    nominal = p.model
    plant = T.Cartpole(mc=nominal.mc, mp=1.2 * nominal.mp, l=nominal.l, g=nominal.g)
    Xr, Ur, dxr = restate(oracle, p, c["Xbar"], c["Ubar"], c["K"], c["d"], c["X0s"][:, :S], plant=plant)
    assert np.abs(Xr - c["ref"][0]).max() > 1e-3, "the heavier pole must move the closed loop"
    Jr, cr = oracle_cost_and_violation(oracle, "cartpole5", Xr, Ur)
    r = T.policy_rollout(p, c["X0s"][:, :S], plant=plant, trajectories=True)
    compare("cartpole plant S=70", r, (Xr, Ur, dxr, Jr, cr))
    r1 = T.policy_rollout(p, c["X0s"][:, :1], plant=plant, trajectories=True)
    compare("cartpole plant S=1", r1, ref_slice((Xr, Ur, dxr, Jr, cr), 1))


# ------------------------------------------------------------------------------------------------ 5. limits
@pytest.mark.parametrize("S", [3, 70])
def test_a_sample_beyond_the_state_limit(S, hip):
    opts = T.SolverOptions(lib=hip, max_state_value=1e2)
    p = configs.cartpole_problem(batch=5, N=31, tf=3.0, lib=hip, options=opts)
    T.iLQRSolver(p).solve()
    Xbar = T.states(p)
    X0s = sample_starts(p, Xbar, 0.05, S)
    clean = T.policy_rollout(p, X0s, trajectories=True)
    np.testing.assert_array_equal(clean.status, 0)
    bad = X0s.copy()
    b, s = 1, S - 1
    bad[b, s, 0] = 1e3
    r = T.policy_rollout(p, bad, trajectories=True)
    assert r.status[b, s] == T.capi.STATE_LIMIT and r.k_limit[b, s] == 1
    assert np.isposinf(r.J[b, s]) and np.isposinf(r.c_max[b, s]) and np.isposinf(r.dx_max[b, s])
    keep = np.ones((5, S), bool); keep[b, s] = False
    for k in ("X", "U", "J", "c_max", "dx_max", "status", "k_limit"):
        np.testing.assert_array_equal(getattr(r, k)[keep], getattr(clean, k)[keep], err_msg=k)


# ------------------------------------------------------------------------------------------------ 6. handle hygiene
def test_refresh_gains_is_expand_plus_backward(hip, oracle):
    for case in ("cartpole5", "quickstart", "quadrotor"):
        c = solved(case, hip, oracle)
        p, X0s = c["p"], c["X0s"][:, :3]
        before = (T.states(p), T.controls(p), [I.get_duals(p, i) for i in range(len(p.constraints))])
        a = T.policy_rollout(p, X0s, alpha=0.3, refresh_gains=True, trajectories=True)
        ga = I.gains(p)
        I.expand(p); I.backwardpass(p)
        gb = I.gains(p)
        b = T.policy_rollout(p, X0s, alpha=0.3, refresh_gains=False, trajectories=True)
        for k in ("K", "d", "dV", "rho"):
            np.testing.assert_array_equal(ga[k], gb[k], err_msg=f"{case} {k}")
        for k in ("X", "U", "J", "c_max", "dx_max", "status", "k_limit"):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{case} {k}")
        after = (T.states(p), T.controls(p), [I.get_duals(p, i) for i in range(len(p.constraints))])
        np.testing.assert_array_equal(before[0], after[0]); np.testing.assert_array_equal(before[1], after[1])
        for (l0, m0), (l1, m1) in zip(before[2], after[2]):
            np.testing.assert_array_equal(l0, l1); np.testing.assert_array_equal(m0, m1)


@pytest.mark.parametrize("kind", ["cartpole_ilqr", "quickstart_al"])
def test_a_solve_after_a_policy_rollout_equals_a_fresh_handle(kind, hip):
    def make():
        if kind == "cartpole_ilqr":
            p = configs.cartpole_problem(batch=70, N=31, tf=3.0, lib=hip)
            return p, T.iLQRSolver(p)
        p = _quickstart(hip, 5)
        return p, T.ALSolver(p)
    pf, sf = make()
    sf.solve()
    ph, sh = make()
    T.rollout(ph)
    rng = np.random.default_rng(3)
    for S in (2, 70):
        T.policy_rollout(ph, T.states(ph)[:, None, 0, :] + 0.05 * rng.standard_normal((ph.B, S, ph.n)), alpha=1.0, trajectories=True)
    sh.solve()
    for k in sf.stats:
        np.testing.assert_array_equal(sh.stats[k], sf.stats[k], err_msg=k)
    np.testing.assert_array_equal(T.states(ph), T.states(pf))
    np.testing.assert_array_equal(T.controls(ph), T.controls(pf))


@pytest.mark.parametrize("case", ["cartpole70", "quadrotor"])
def test_parity_under_the_guard(case, hip, oracle, monkeypatch):
    """TRAJOPT_GUARD=1: the arrays of the policy rollout sit between red zones like every other array of the handle; both lane maps, the
    chunked download included, leave them intact and give the unguarded numbers."""
    c = solved(case, hip, oracle)
    monkeypatch.setenv("TRAJOPT_GUARD", "1")
    p = CASES[case]["build"](hip, CASES[case]["B"])
    T.initial_states(p, c["Xbar"]); T.initial_controls(p, c["Ubar"])
    monkeypatch.setenv("TRAJOPT_POLICY_CHUNK_WAVES", "2")
    for S in (3, 70, 64):        # (the per-sample arrays and the staging are re-sized as S grows)
        r = T.policy_rollout(p, c["X0s"][:, :S], trajectories=True)
        compare(f"{case} guard S={S}", r, ref_slice(c["ref"], S))


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors(hip, oracle):
    c = solved("cartpole5", hip, oracle)
    p = c["p"]
    x0s = np.ascontiguousarray(c["X0s"][:, :2])
    out = T.capi.PolicyResult()
    with pytest.raises(T.ArgumentError, match="S must be"):
        p._call("policy_rollout", 0, p._pd(x0s), None, C.byref(out))
    with pytest.raises(ValueError, match="x0s is NULL"):
        p._call("policy_rollout", 2, None, None, C.byref(out))
    with pytest.raises(ValueError, match="out is NULL"):
        p._call("policy_rollout", 2, p._pd(x0s), None, None)
    p._call("policy_rollout", 2, p._pd(x0s), None, C.byref(out))     # NULL options = the defaults; every output may be NULL
    # a plant with another attitude representation: refused by the library (same dimensions, so the host check lets it through)
    q = configs.quadrotor_problem(batch=2, N=11, tf=0.5, lib=hip)
    T.rollout(q)
    o = T.capi.PolicyOpts()
    pp = np.zeros(16); pp[:11] = q.model.params(); pp[10] = 1.0
    o.refresh_gains, o.plant_params = 1, q._pd(pp)
    xq = np.ascontiguousarray(T.states(q)[:, None, 0, :])
    with pytest.raises(T.ArgumentError, match="attitude representation"):
        q._call("policy_rollout", 1, q._pd(xq), C.byref(o), C.byref(out))
    with pytest.raises(T.ArgumentError):
        T.policy_rollout(q, xq, plant=T.Quadrotor(rotation="mrp"))
    with pytest.raises(T.ArgumentError):
        T.policy_rollout(q, xq, plant=T.Cartpole())
    # while a solve is in flight the handle refuses the call like any other
    big = configs.quadrotor_problem(batch=256, N=101, tf=5.0, lib=hip)
    s = T.iLQRSolver(big)
    s.solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="in flight"):
            T.policy_rollout(big, np.zeros((big.B, 1, big.n)))
    finally:
        s.wait()
