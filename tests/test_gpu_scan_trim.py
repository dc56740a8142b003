"""The trimmed round loop of the scan backward pass (k_scan.h, TRIM: the last scan round computes the value part (eta, J) alone and
fetches only the partner's (J, eta); lanes past lane 63's reach read lane 63 as it is) against the untrimmed instance kept behind
TRAJOPT_SCAN_TRIM=0.  Same expressions in the same order for everything that is kept: gains, expected improvement, regularisation
and whole solves must be the same BYTES (tobytes(): -0.0 != +0.0), over every round count of the scan (N = 2: no round; N = 3, 4: the
only round is the last one; ... N = 126: six), both sides of each change, m = 1 and m = 2, one and two tiles of trajectories."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

pytestmark = pytest.mark.gpu

HORIZONS = [2, 3, 4, 5, 6, 9, 10, 17, 18, 33, 34, 65, 66, 101, 125, 126]


@pytest.fixture(autouse=True)
def scan_everywhere(monkeypatch):
    monkeypatch.setenv("TRAJOPT_SCAN", "2")  # (read when a handle is made: the phase API runs the solve loop's scan kernel too)


def _cartpole(hip, batch, N, **kw):
    return configs.cartpole_problem(batch=batch, N=N, tf=0.05 * (N - 1), lib=hip, **kw)


def _di(hip, batch, N):
    model = T.DoubleIntegrator(1.0, 2)
    obj = T.LQRObjective(np.array([1.0, 2.0, 0.5, 0.3]), np.array([0.1, 0.2]), 10 * np.ones(4), np.array([1.0, 2.0, 0, 0]), N)
    p = T.Problem(model, obj, np.array([0.2, -0.1, 0.0, 0.3]), 0.1 * (N - 1), batch=batch, lib=hip)
    p.set_initial_state(np.array([0.2, -0.1, 0.0, 0.3]) + 0.3 * np.random.default_rng(batch + N).standard_normal((batch, 4)))
    T.initial_controls(p, np.array([0.1, -0.05]))
    return p


MODELS = {"cartpole": _cartpole, "di2": _di}


def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _backward(p, trim, monkeypatch):
    monkeypatch.setenv("TRAJOPT_SCAN_TRIM", trim)  # (read at every launch of the scan kernel)
    I.expand(p); I.backwardpass(p)
    return I.gains(p)


def _compare_gains(p1, p0, monkeypatch, what):
    g1, g0 = _backward(p1, "1", monkeypatch), _backward(p0, "0", monkeypatch)
    for k in ("K", "d", "dV", "rho"):
        _same_bytes(g1[k], g0[k], f"{what}: {k}")
    assert np.isfinite(g1["K"]).all() and np.abs(g1["K"]).max() > 0
    return g1


@pytest.mark.parametrize("N", HORIZONS)
def test_gains_are_the_same_bytes(N, hip, monkeypatch):
    for name, build in MODELS.items():
        for batch in (9, 70):
            p1, p0 = build(hip, batch, N), build(hip, batch, N)
            for it in range(4):  # the initial guess and three further iterates
                if it == 0:
                    T.rollout(p1); T.rollout(p0)
                _compare_gains(p1, p0, monkeypatch, f"{name} B={batch} N={N} iterate {it}")
                ls1, J1 = I.forwardpass(p1)
                ls0, J0 = I.forwardpass(p0)
                _same_bytes(ls1, ls0, "line-search index"); _same_bytes(J1, J0, "cost")


def test_pending_regularisation_takes_the_untouched_sequential_pass(hip, monkeypatch):
    mk = lambda: configs.cartpole_problem(batch=33, lib=hip, options=T.SolverOptions(lib=hip, bp_reg_initial=5.0))
    p1, p0 = mk(), mk()
    T.rollout(p1); T.rollout(p0)
    _compare_gains(p1, p0, monkeypatch, "bp_reg_initial=5")


def _solve(build, trim, monkeypatch):
    monkeypatch.setenv("TRAJOPT_SCAN_TRIM", trim)
    p = build()
    s = T.iLQRSolver(p, iterations=25).solve()
    return {k: v.copy() for k, v in s.stats.items()}, T.states(p), T.controls(p)


@pytest.mark.parametrize("N", [21, 101])
@pytest.mark.parametrize("name", list(MODELS))
def test_solves_are_the_same_bytes(name, N, hip, monkeypatch):
    st1, X1, U1 = _solve(lambda: MODELS[name](hip, 9, N), "1", monkeypatch)
    st0, X0, U0 = _solve(lambda: MODELS[name](hip, 9, N), "0", monkeypatch)
    assert set(st1) == set(st0) and st1["iterations"].max() >= 1
    for k in st1:
        _same_bytes(np.asarray(st1[k]), np.asarray(st0[k]), f"{name} N={N}: stat {k}")
    _same_bytes(X1, X0, "states"); _same_bytes(U1, U0, "controls")


def test_two_solves_in_flight_equal_the_solves_run_alone(hip):
    """A depth-2 pipeline of two Cartpole batches of 70: scan waves of one solve share the chip with the other solve's forward pass,
    where the scan wave's static priority acts.  Priority changes no arithmetic: every job equals the solve that ran alone."""
    def mk():
        return T.iLQRSolver(configs.cartpole_problem(batch=70, lib=hip), iterations=25)
    ref = mk()
    u0 = T.controls(ref.prob)[0, 0].copy()
    ref.solve()
    want = ({k: v.copy() for k, v in ref.stats.items()}, T.states(ref.prob), T.controls(ref.prob))
    got = {}
    pipe = T.SolvePipeline([mk(), mk()], admit_below=70,
                           on_done=lambda job, s: got.__setitem__(job, ({k: v.copy() for k, v in s.stats.items()}, T.states(s.prob), T.controls(s.prob))))
    for _ in range(4):
        pipe.submit(lambda p: T.initial_controls(p, u0))
    pipe.drain()
    assert sorted(got) == [0, 1, 2, 3]
    for job, (st, X, U) in got.items():
        for k in want[0]:
            _same_bytes(np.asarray(st[k]), np.asarray(want[0][k]), f"job {job}: stat {k}")
        _same_bytes(X, want[1], f"job {job}: states"); _same_bytes(U, want[2], f"job {job}: controls")
