"""List mode of the two-wave forward pass (csrc/fwd_list.h): the scan kernel of every batch step lists the active trajectories and
k_forward2 takes its trajectories from that list, workgroups for the trajectories still active only.  Which lane works on which
trajectory changes nothing in its arithmetic, so whole solves with TRAJOPT_FWD_LIST=1 must be the same BYTES (tobytes(): -0.0 != +0.0)
as with TRAJOPT_FWD_LIST=0, the forward pass's fixed map: states, controls, gains and every stats array.

The inputs make the list work — checked on the =0 run's own iteration counts: the batch finishes at three or more distinct steps, and
at some step the active set is non-empty, smaller than the batch and not a prefix of it (neither can hold for B = 1, which is compared
all the same).  The Cartpole batches drain unevenly by themselves.  A linear model with a quadratic cost converges in two iterations
from anywhere, so the double integrators get three interleaved classes: trajectories left as they are (two iterations), trajectories that
start on their own optimum — the controls a solve on the fixed map found for them — (one), and trajectories whose start state lies
beyond max_state_value (ended by the initial rollout, none)."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

import failure_cases

pytestmark = pytest.mark.gpu
S = T.capi


def _snapshot(solver):
    p = solver.prob
    out = {f"stat {k}": np.array(v).copy() for k, v in solver.stats.items()}
    out["states"], out["controls"] = T.states(p), T.controls(p)
    out.update({f"gains {k}": v for k, v in I.gains(p).items()})
    return out


def _same_bytes(got, want, what):
    assert set(got) == set(want)
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {k}"


def _solve(build, switch, monkeypatch, Solver=T.iLQRSolver, **kw):
    monkeypatch.setenv("TRAJOPT_FWD_LIST", switch)  # (read at the start of every solve)
    s = Solver(build(), **kw)
    s.solve()
    return _snapshot(s)


def _list_is_exercised(iterations, B):
    """From the iteration counts of a solve: the batch finishes at >= 3 distinct steps; at some step the active set is non-empty, smaller
    than B and not a prefix of the batch.  (A trajectory with i iterations is active in the steps 0 .. i-1.)"""
    its = np.asarray(iterations)
    distinct = len(set(its.tolist())) >= 3
    ragged = False
    for step in range(int(its.max())):
        act = its > step
        na = int(act.sum())
        ragged |= 0 < na < B and not bool(act[:na].all())
    return distinct, ragged


def _compare(build, B, monkeypatch, what, **kw):
    want = _solve(build, "0", monkeypatch, **kw)
    got = _solve(build, "1", monkeypatch, **kw)
    if B > 1:
        distinct, ragged = _list_is_exercised(want["stat iterations"], B)
        assert distinct, f"{what}: the batch finishes at fewer than three distinct steps: {sorted(set(want['stat iterations'].tolist()))}"
        assert ragged, f"{what}: the active set is never a proper, non-prefix part of the batch"
    assert want["stat iterations"].max() >= 1 and np.isfinite(want["states"]).all()
    _same_bytes(got, want, what)
    return want


def _cartpole(hip, B, N, **kw):
    return configs.cartpole_problem(batch=B, N=N, tf=0.05 * (N - 1), lib=hip, **kw)


@pytest.mark.parametrize("B", [1, 17, 65, 200])
@pytest.mark.parametrize("N", [21, 22])  # even and odd block counts of the scan
def test_cartpole_solves_are_the_same_bytes(N, B, hip, monkeypatch):
    _compare(lambda: _cartpole(hip, B, N), B, monkeypatch, f"cartpole N={N} B={B}", iterations=25)


def _double_integrator(hip, D, B, N=21):
    n, m = 2 * D, D
    rng = np.random.default_rng(100 + D)
    obj = T.LQRObjective(rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 0.3, m), 10 * np.ones(n), np.concatenate([np.ones(D), np.zeros(D)]), N)
    p = T.Problem(T.DoubleIntegrator(1.0, D), obj, np.zeros(n), 0.1 * (N - 1), batch=B, lib=hip)
    p.set_initial_state(0.5 * np.random.default_rng(B + N + D).standard_normal((B, n)))
    T.initial_controls(p, np.full(m, 0.05))
    return p


def _hybrid(hip, B, N=11):
    models = T.HybridDoubleIntegrator(1.3, 5).models(N)
    nx, nu = T.dims(models)
    rng = np.random.default_rng(5)
    costs = [T.LQRCost(rng.uniform(0.5, 2.0, n), rng.uniform(0.05, 0.3, m), rng.uniform(-1, 1, n), rng.uniform(-0.2, 0.2, m)) for n, m in zip(nx, nu)]
    x0 = np.array([0.5, -0.4, 0.2, 0.1])
    p = T.Problem(models, T.Objective(costs), x0, 2.0, constraints=T.ConstraintList(models), batch=B, lib=hip)
    p.set_initial_state(x0 + 0.3 * np.random.default_rng(B).standard_normal((B, 4)))
    return p


def _three_classes(base, B, monkeypatch):
    """-> a builder of `base`'s problem with the classes of the module docstring interleaved over the batch (b mod 3)"""
    monkeypatch.setenv("TRAJOPT_FWD_LIST", "0")  # the reference path alone picks the inputs
    p = base()
    x0, U0 = np.array(p.x0, copy=True), T.controls(p)
    T.iLQRSolver(p, iterations=25).solve()
    b = np.arange(B)
    U0[b % 3 == 1] = T.controls(p)[b % 3 == 1]
    x0[b % 3 == 2] = 0.0
    x0[b % 3 == 2, 0] = 1e9  # (max_state_value: 1e8)

    def build():
        q = base()
        q.set_initial_state(x0)
        T.initial_controls(q, U0)
        return q
    return build


@pytest.mark.parametrize("name,B", [("di1", 65), ("di2", 65), ("hybrid", 17)])
def test_linear_models_are_the_same_bytes(name, B, hip, monkeypatch):
    base = {"di1": lambda: _double_integrator(hip, 1, B), "di2": lambda: _double_integrator(hip, 2, B), "hybrid": lambda: _hybrid(hip, B)}[name]
    want = _compare(_three_classes(base, B, monkeypatch), B, monkeypatch, name, iterations=25)
    assert (want["stat status"][2::3] == S.STATE_LIMIT).all() and (want["stat iterations"][2::3] == 0).all()


@pytest.mark.parametrize("case,status", [("cartpole_regmax", S.REGULARIZATION_MAX), ("cartpole_no_progress", S.NO_PROGRESS)])
def test_failing_batches_are_the_same_bytes(case, status, hip, monkeypatch):
    """Batches of tests/failure_cases.py: trajectories that end in REGULARIZATION_MAX (cartpole_regmax: part of the batch restarts its
    backward pass — the scan wave's in-wave sequential fallback — and part of that runs into bp_reg_max) and in NO_PROGRESS (failed
    line searches from the first pass on) next to trajectories that go on: whoever leaves is settled, whoever stays keeps its slot."""
    c = failure_cases.CASES[case]
    want = _compare(lambda: c.build(hip), 70, monkeypatch, case)
    assert (want["stat status"] == status).any() and len(set(want["stat status"].tolist())) >= 2
    if case == "cartpole_regmax":  # some trajectory went through the sequential fallback and still finished its solve otherwise
        fp = c.first_pass(hip, forward=False)
        assert ((fp["rho"] > 0) & ~fp["bpfail"]).any()


def test_trajectories_ended_by_the_initial_rollout(hip, monkeypatch):
    """A low max_state_value: the initial rollout ends part of the batch (STATE_LIMIT, no iteration) before step 0, so the first list is
    shorter than the batch and its length comes from where the rollout decides."""
    N, B = 21, 65

    def build():
        p = _cartpole(hip, B, N, options=T.SolverOptions(lib=hip, max_state_value=0.4))
        return p
    want = _compare(build, B, monkeypatch, "max_state_value", iterations=25)
    ended = want["stat status"] == S.STATE_LIMIT
    assert 0 < ended.sum() < B and (want["stat iterations"][ended] == 0).all() and (want["stat iterations"][~ended] >= 1).all()


def test_two_pipelined_handles_equal_the_unpipelined_solve(hip, monkeypatch):
    monkeypatch.setenv("TRAJOPT_FWD_LIST", "1")

    def mk():
        return T.iLQRSolver(_cartpole(hip, 70, 21), iterations=25)
    ref = mk()
    u0 = T.controls(ref.prob)[0, 0].copy()
    ref.solve()
    want = _snapshot(ref)
    assert all(_list_is_exercised(want["stat iterations"], 70))
    got = {}
    pipe = T.SolvePipeline([mk(), mk()], admit_below=70, on_done=lambda job, s: got.__setitem__(job, _snapshot(s)))
    for _ in range(4):
        pipe.submit(lambda p: T.initial_controls(p, u0))
    pipe.drain()
    assert sorted(got) == [0, 1, 2, 3]
    for job, snap in got.items():
        _same_bytes(snap, want, f"job {job}")


@pytest.mark.parametrize("first", ["0", "1"])
def test_resolve_with_the_switch_flipped_equals_a_fresh_handle(first, hip, monkeypatch):
    """The mode is armed per solve: a handle that solved on one map solves again on the other and equals a fresh handle."""
    mk = lambda: _cartpole(hip, 65, 22)
    monkeypatch.setenv("TRAJOPT_FWD_LIST", first)
    s = T.iLQRSolver(mk(), iterations=25)
    u0 = T.controls(s.prob)[0, 0].copy()
    s.solve()
    one = _snapshot(s)
    monkeypatch.setenv("TRAJOPT_FWD_LIST", "1" if first == "0" else "0")
    T.initial_controls(s.prob, u0)
    s.solve()
    two = _snapshot(s)
    fresh = _solve(mk, "1" if first == "0" else "0", monkeypatch, iterations=25)
    _same_bytes(two, fresh, "re-solve vs fresh handle")
    _same_bytes(two, one, "re-solve vs the handle's first solve")
