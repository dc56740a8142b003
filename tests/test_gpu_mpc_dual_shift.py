"""to_mpc_shift_duals on the MI355X (csrc/k_mpc.h k_mpc_shift_duals): the multipliers of a handle moved with the plan, or
reset, per trajectory.  The kernel only copies, so every comparison is equality of BITS with the numpy restatement below (``shift_duals``),
penalties included; under TRAJOPT_GUARD=1 no red zone is touched; the refusals are tested through the C call.  A library without the
entry point FAILS every test here (no skip)."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

pytestmark = pytest.mark.gpu
cap = T.capi
DINT_XF = np.array([1.0, 2.0, 0.0, 0.0])


@pytest.fixture(autouse=True)
def _symbol_is_there(hip):
    assert "mpc_shift_duals" in hip._fn, "libtrajopt_hip.so does not export to_mpc_shift_duals"


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def all_duals(p):
    return [I.get_duals(p, i) for i in range(len(p.constraints))]


def shift_duals(lam, s, tail="hold", action=None):
    """The numpy restatement for one constraint: lam [B, nk, p] -> the shifted copy.  action [B] of 0 / 1 / 2 (None: 1 for all)."""
    B, nk, _ = lam.shape
    moved = np.zeros_like(lam)
    for j in range(nk):
        if j + s < nk:
            moved[:, j] = lam[:, j + s]
        elif tail == "hold":
            moved[:, j] = lam[:, nk - 1]
    act = np.ones(B, int) if action is None else np.asarray(action)
    out = np.where((act == 1)[:, None, None], moved, lam)
    out[act == 2] = 0.0
    return out


N_SHIFT = 11


def shift_problem(lib, B, N=N_SHIFT):
    """dint with a BoundConstraint on knots 1 .. N-1 (p = 6), a control bound on knots 4 .. 8 (p = 4) and the goal at N (p = 4, one knot)."""
    n, m = 4, 2
    obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 100 * np.ones(n), DINT_XF, N)
    cons = T.ConstraintList(n, m, N)
    T.add_constraint(cons, T.BoundConstraint(n, m, x_max=[np.inf, np.inf, np.inf, 0.7], x_min=[-0.5, -np.inf, -np.inf, -np.inf],
                                             u_max=[1.2, 1.2], u_min=[-1.2, -1.2]), (1, N - 1))
    T.add_constraint(cons, T.BoundConstraint(n, m, u_max=[1.0, 1.1], u_min=[-1.0, -1.1]), (4, 8))
    T.add_constraint(cons, T.GoalConstraint(DINT_XF), N)
    p = T.Problem(T.DoubleIntegrator(1.0, 2), obj, np.zeros(n), 1.0, xf=DINT_XF, constraints=cons, batch=B, lib=lib)
    assert [(c.p, b - a + 1) for c, (a, b) in zip(p.constraints, p.constraints.inds)] == [(6, N - 1), (4, 5), (4, 1)]
    return p


def _shift_cases(p, rng, cases):
    B, mu0 = p.B, T.iLQRSolver(p).opts.penalty_initial
    for s, tail, with_action in cases:
        before = []
        for i, (lam, mu) in enumerate(all_duals(p)):
            lam, mu = rng.standard_normal(lam.shape), rng.uniform(1.0, 1e4, mu.shape)
            I.set_duals(p, i, lam, mu)
            before.append((lam, mu))
        action = rng.integers(0, 3, B).astype(np.int32) if with_action else None
        T.mpc_shift_duals(p, s, tail, action)
        for i, ((lam, mu), (lam2, mu2)) in enumerate(zip(before, all_duals(p))):
            assert same(lam2, shift_duals(lam, s, tail, action)), f"lambda: s {s} tail {tail} constraint {i}"
            assert same(mu2, mu if action is None else np.where(action == cap.MPC_DUAL_RESET, mu0, mu)), f"mu: s {s} tail {tail} constraint {i}"


@pytest.mark.parametrize("B", [70, 130])
def test_shift_equals_the_numpy_restatement(B, hip):
    p = shift_problem(hip, B)
    _shift_cases(p, np.random.default_rng(B), [(s, tail, True) for s in (1, 4, 5, 9) for tail in ("hold", "zero")] + [(4, "hold", False)])
    # all LEAVE stores nothing; strings name the actions
    before = all_duals(p)
    T.mpc_shift_duals(p, 2, action=["leave"] * B)
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(before, all_duals(p)))


def test_shift_runs_clean_under_the_guard(hip, monkeypatch):
    monkeypatch.setenv("TRAJOPT_GUARD", "1")       # red zones around every array of the handle, checked by the entry point
    p = shift_problem(hip, 130)
    _shift_cases(p, np.random.default_rng(5), [(1, "hold", True), (9, "zero", True), (5, "hold", False)])


def _raw(p, shift, tail, action=None):
    p._call("mpc_shift_duals", shift, tail, None if action is None else p._pi(np.ascontiguousarray(action, dtype=np.int32)))


def test_refusals_through_the_c_call(hip):
    p = shift_problem(hip, 5)
    rng = np.random.default_rng(1)
    for i, (lam, mu) in enumerate(all_duals(p)):
        I.set_duals(p, i, rng.standard_normal(lam.shape), rng.uniform(1, 9, mu.shape))
    before = all_duals(p)
    rows = [((0, 0), T.ArgumentError, r"to_mpc_shift_duals: shift must be in 1 \.\. N-2 = 9; got 0"), ((N_SHIFT - 1, 0), T.ArgumentError, "shift must be"),
            ((-3, 0), T.ArgumentError, "shift must be"), ((1, 2), T.ArgumentError, "to_mpc_shift_duals: tail must be"), ((1, -1), T.ArgumentError, "tail must be"),
            ((1, 0, [1, 1, 3, 1, 1]), T.ArgumentError, "action of trajectory 2 is 3"), ((1, 1, [1, 1, 1, 1, -1]), T.ArgumentError, "action of trajectory 4 is -1")]
    for args, err, match in rows:
        with pytest.raises(err, match=match):
            _raw(p, *args)
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(before, all_duals(p))), "a refused call changed the duals"
    # a handle without constraints: TO_OK, nothing to do
    q = configs.cartpole_problem(batch=3, N=11, tf=1.0, lib=hip)
    T.mpc_shift_duals(q, 2)


def test_models_that_cannot_shift_are_refused_by_name(hip):
    from test_hybrid_dims import hybrid_problem
    hyb = hybrid_problem(hip, batch=3)[0]
    base = configs.cartpole_problem(batch=3, N=11, tf=1.0, constrained=True, lib=hip)
    T.rollout(base)
    inf = T.InfeasibleProblem(base, T.states(base), R_inf=1.0)
    for prob, name in ((hyb, "hybrid double integrator"), (inf, r"InfeasibleModel \(Cartpole\)")):
        with pytest.raises(T.UnsupportedError, match="to_mpc_shift_duals: not available for the " + name + ".*cannot shift their plan"):
            _raw(prob, 1, 0)


def test_a_solve_in_flight_refuses(hip):
    import constraint_limit_fleets as F
    p = F.spec("dint", 70).batch(hip)
    s = T.ALSolver(p, **F.AL_KW)
    s.solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="an asynchronous solve is in flight"):
            T.mpc_shift_duals(p, 1)
    finally:
        s.wait()
    T.mpc_shift_duals(p, 1)
