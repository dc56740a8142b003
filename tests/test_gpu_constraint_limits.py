"""Per-trajectory constraint limits on the MI355X (to_set_constraint_limits_batch): one handle whose trajectories each have
their own BoundConstraint bounds or second-order-cone value, against B single-trajectory ORACLE problems built with trajectory b's limit
(tests/constraint_limit_fleets.py; vetted on the oracle alone by tests/test_constraint_limits_oracle.py).  Tolerances are those of
tests/test_goal_batch.py::test_per_trajectory_goal_constraints_on_gpu / test_per_trajectory_linear_rhs_on_gpu; integers bit-exact.

How far inside its limits a solve ends: the polished (ALTRO) trajectories within 2e-6; the AL solves run with constraint_tolerance = 1e-4 and
the oracle's own end up to 1.6e-4 outside in the Euclidean measure taken here, so they are held to 2e-4 (the bound test_goal_batch.py puts
on its AL solves) — see tests/test_constraint_limits_oracle.py."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import constraint_limit_fleets as F

pytestmark = pytest.mark.gpu

FLEETS = [("cartpole", 70, None), ("cartpole_split", 70, None), ("cartpole", 300, "lane"), ("dint", 40, None), ("quadrotor", 24, None)]
IDS = [f"{n}-{B}" + (f"-{e}" if e else "") for n, B, e in FLEETS]
INSIDE = {"al": 2e-4, "altro": 2e-6}


def _env(monkeypatch, env):
    if env == "lane":  # the lane path with compaction, as test_per_trajectory_goal_constraints_on_gpu runs it
        monkeypatch.setenv("TRAJOPT_BACKWARD", "lane"); monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_MIN", "1")


def _path(p):
    info = np.zeros(8, dtype=np.int32)
    p._call("solver_path", p._pi(info))
    return list(info)


def _bits(p, s):
    return (T.states(p), T.controls(p)) + tuple(s.stats[k].copy() for k in ("iterations", "iterations_outer", "iterations_pn", "status", "cost", "c_max"))


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=what)


@pytest.mark.parametrize("name,B,env", FLEETS, ids=IDS)
def test_phases(name, B, env, hip, oracle, monkeypatch):
    _env(monkeypatch, env)
    s = F.spec(name, B)
    ref = F.reference_phases(name, B, oracle)
    ph = s.batch(hip)
    r = F.phases(ph, s.con_id)
    np.testing.assert_allclose(r.c, ref.c, rtol=1e-11, atol=1e-12)
    np.testing.assert_array_equal(r.jac, ref.jac)
    np.testing.assert_allclose(r.viol, ref.viol, rtol=1e-11)
    np.testing.assert_allclose(r.al, ref.al, rtol=1e-11)
    np.testing.assert_allclose(r.K, ref.K, rtol=1e-6, atol=1e-8); np.testing.assert_allclose(r.d, ref.d, rtol=1e-6, atol=1e-8)
    np.testing.assert_array_equal(r.ls, ref.ls); np.testing.assert_allclose(r.J, ref.J, rtol=1e-9)
    # the limits matter at this point: the shared nominal limit gives other constraint values
    shared = s.shared(hip)
    T.rollout(shared)
    assert np.abs(T.evaluate_constraints(shared, s.con_id) - ref.c).max() > 1e-2


@pytest.mark.parametrize("solver", ["al", "altro"])
@pytest.mark.parametrize("name,B,env", FLEETS, ids=IDS)
def test_solves(name, B, env, solver, hip, oracle, monkeypatch):
    _env(monkeypatch, env)
    s = F.spec(name, B)
    ref = F.reference_solve(name, B, solver, oracle)
    Solver, kw = s.solvers[solver]
    ph = s.batch(hip)
    sh = Solver(ph, **kw).solve()
    F.assert_solve_parity_fleet(sh, ph, ref, s.shared(oracle), rtol=1e-5 if solver == "al" else 1e-6)
    ok = sh.stats["status"] == F.OK
    assert ok.mean() > 0.9
    out, gap = s.margins(T.states(ph), T.controls(ph))
    print(f"\n{name} B={B} {solver}: leaves its limits by <= {out[ok].max():.2e}, worst approach {gap.max():.2e}")
    assert out[ok].max() < INSIDE[solver]          # every successful trajectory inside ITS limits
    assert gap.max() < 1e-3                        # ... and its control touches its own limit


def test_setter_semantics(hip, oracle):
    """Getter round trip; to_set_constraint on a flagged id returns it to shared limits; after to_clear_... a solve is bit-identical to one on a
    fresh handle; setting other limits a second time gives what a fresh handle with those limits gives, bit for bit."""
    s = F.spec("dint", 40)
    p = s.shared(hip)
    shared_limits = np.tile([0.7, 1.2, 1.2, -0.5, -1.2, -1.2], (40, 1))
    np.testing.assert_array_equal(T.get_constraint_limits_batch(p, 0), shared_limits)       # nothing set: the descriptor's values, repeated
    fresh = _bits(p, T.ALSolver(p, **F.AL_KW).solve())
    s.set_limits(p)
    np.testing.assert_array_equal(T.get_constraint_limits_batch(p, 0), s.limits)
    first = _bits(p, T.ALSolver(p, **F.AL_KW).solve())
    assert not np.array_equal(first[1], fresh[1])
    # a second set of limits on the same handle == a fresh handle with those limits
    other = s.limits[::-1].copy()
    T.set_constraint_limits_batch(p, 0, other)
    np.testing.assert_array_equal(T.get_constraint_limits_batch(p, 0), other)
    q = s.shared(hip)
    T.set_constraint_limits_batch(q, 0, other)
    for prob in (p, q):
        T.initial_controls(prob, np.zeros(2)); T.rollout(prob)
    _same_bits(_bits(p, T.ALSolver(p, **F.AL_KW).solve()), _bits(q, T.ALSolver(q, **F.AL_KW).solve()), "second set of limits vs fresh handle")
    # to_set_constraint on the flagged constraint: shared limits again (the getter says so, the solve is the fresh one)
    con = p.constraints.constraints[0]
    a, b = p.constraints.inds[0]
    d = con._desc(a, b)
    p._call("set_constraint", 0, T.capi.C.byref(d))
    np.testing.assert_array_equal(T.get_constraint_limits_batch(p, 0), shared_limits)
    T.initial_controls(p, np.zeros(2)); T.rollout(p)
    _same_bits(_bits(p, T.ALSolver(p, **F.AL_KW).solve()), fresh, "after to_set_constraint")
    # to_clear_...: the whole handle back on its descriptors
    s.set_limits(p)
    T.clear_constraint_limits_batch(p)
    np.testing.assert_array_equal(T.get_constraint_limits_batch(p, 0), shared_limits)
    T.initial_controls(p, np.zeros(2)); T.rollout(p)
    _same_bits(_bits(p, T.ALSolver(p, **F.AL_KW).solve()), fresh, "after to_clear_constraint_limits_batch")
    fresh_path = _path(s.shared(hip))
    assert _path(p) == fresh_path
    s.set_limits(p)
    assert _path(p)[1] == 0 and _path(p)[5] == 0       # flagged: no fused cooperative kernel, no scan kernel (the route of a cp handle)
    T.clear_constraint_limits_batch(p)
    assert _path(p) == fresh_path


def test_refusals(hip):
    s = F.spec("quadrotor", 24)
    p = F.quadrotor_problem(hip, 3, N=11, tf=0.5)
    gi = next(i for i, c in enumerate(p.constraints.constraints) if isinstance(c, T.GoalConstraint))
    with pytest.raises(T.UnsupportedError, match="BoundConstraint .its bounds. and NormConstraint with SecondOrderCone .its value. only"):
        p._call("set_constraint_limits_batch", gi, p._pd(np.zeros(3 * 9)))
    with pytest.raises(T.UnsupportedError, match="only"):
        T.get_constraint_limits_batch(p, gi)
    with pytest.raises(AssertionError, match="Value must be greater than or equal to zero .trajectory 1."):
        T.set_constraint_limits_batch(p, 0, [6.0, -1.0, 6.0])
    with pytest.raises(T.ArgumentError, match="not finite"):
        T.set_constraint_limits_batch(p, 0, [6.0, np.nan, 6.0])
    for bad in (-1, len(p.constraints)):
        with pytest.raises(T.ArgumentError, match="constraint id out of range"):
            p._call("set_constraint_limits_batch", bad, p._pd(np.zeros(3)))
        with pytest.raises(T.ArgumentError, match="constraint id out of range"):
            p._call("get_constraint_limits_batch", bad, p._pd(np.zeros(3)))
    np.testing.assert_array_equal(T.get_constraint_limits_batch(p, 0), np.full((3, 1), 6.0))    # a refused call changes nothing
    # the quadratic form of NormConstraint stays refused, by name
    from trajectoryoptimization_jl_amd import configs
    n, m = 13, 4
    cons = T.ConstraintList(n, m, 11)
    T.add_constraint(cons, T.NormConstraint(n, m, 6.0, T.Inequality(), "control"), (1, 10))
    pq = configs.quadrotor_problem(batch=3, N=11, tf=0.5, lib=hip)
    pq = T.Problem(pq.model, pq.obj, np.zeros(n), 0.5, xf=pq.xf, constraints=cons, batch=3, lib=hip)
    with pytest.raises(T.UnsupportedError, match="SecondOrderCone"):
        T.set_constraint_limits_batch(pq, 0, [6.0, 5.0, 4.0])
    # inverted bound in one trajectory
    c = F.cartpole_problem(hip, 3, N=11, tf=0.5)
    with pytest.raises(T.ArgumentError, match="Upper bounds must be greater than or equal to lower bounds .trajectory 2."):
        T.set_constraint_limits_batch(c, 0, np.array([[3.0, -3.0], [2.0, -2.0], [-1.0, 1.0]]))
    # to_set_constraint_params_batch keeps refusing both kinds, in its own words
    with pytest.raises(T.UnsupportedError, match="per-trajectory constraint parameters: GoalConstraint .its target. and LinearConstraint .its b. only"):
        T.set_constraint_params_batch(c, 0, np.zeros((3, 2)))
    # solve in flight
    big = s.shared(hip)
    solver = T.ALSolver(big, **F.AL_KW)
    solver.solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="asynchronous solve is in flight"):
            T.set_constraint_limits_batch(big, 0, s.limits)
        with pytest.raises(T.ArgumentError, match="asynchronous solve is in flight"):
            T.clear_constraint_limits_batch(big)
    finally:
        solver.wait()


def test_combination_with_plants_and_goals(hip, oracle):
    """Plants (to_set_model_params_batch), goals with GoalConstraint targets (set_goal_state) and limits, all per trajectory, against singles
    built with all three; either order of the setters gives the same bits."""
    B = 70
    models, Xf, up, dn = F.combo(B)
    ref = F.combo_reference(oracle)

    def build(order):
        p = F.cartpole_problem(hip, B)
        for what in order:
            if what == "plants":
                T.set_model_params(p, models)
            elif what == "goals":
                T.set_goal_state(p, Xf)
            else:
                T.set_bounds_batch(p, 0, u_max=up[:, None], u_min=dn[:, None])
        return p
    pa = build(("plants", "goals", "limits"))
    sa = T.ALTROSolver(pa).solve()
    po = F.cartpole_problem(oracle, B)
    F.assert_solve_parity_fleet(sa, pa, ref, po, rtol=1e-6)
    ok = sa.stats["status"] == F.OK
    assert ok.mean() > 0.9
    u = T.controls(pa)[:, :, 0]
    assert np.maximum(u - up[:, None], dn[:, None] - u).max(axis=1)[ok].max() < 2e-6
    assert np.abs(T.states(pa)[ok][:, -1, :] - Xf[ok]).max() < 1e-5
    pb = build(("limits", "goals", "plants"))
    _same_bits(_bits(pa, sa), _bits(pb, T.ALTROSolver(pb).solve()), "order of the setters")


def test_policy_rollout_reports_the_violation_of_each_trajectorys_own_bound(hip, oracle):
    """to_policy_rollout with S = 2 on the Cartpole fleet after a solve: c_max of every sample equals the oracle's max_violation of the CPU
    restatement (tests/test_gpu_policy_rollout.py restate) evaluated on a problem built with the trajectory's own bound."""
    from test_gpu_policy_rollout import restate, sample_starts
    B, S = 70, 2
    s = F.spec("cartpole", B)
    p = s.batch(hip)
    T.ALSolver(p, **F.AL_KW).solve()
    I.expand(p); I.backwardpass(p)
    g = I.gains(p)
    Xbar, Ubar = T.states(p), T.controls(p)
    X0s = sample_starts(p, Xbar, 0.05, S)
    r = T.policy_rollout(p, X0s, trajectories=True)
    Xr, Ur, _ = restate(oracle, p, Xbar, Ubar, g["K"], g["d"], X0s)
    cr = np.zeros((B, S))
    for b in range(B):
        q = F.cartpole_problem(oracle, S, u_max=s.u_max[b], u_min=s.u_min[b])
        T.initial_states(q, Xr[b]); T.initial_controls(q, Ur[b])
        cr[b] = T.max_violation(q)
    q = F.cartpole_problem(oracle, B * S)
    T.initial_states(q, Xr.reshape(B * S, *Xr.shape[2:])); T.initial_controls(q, Ur.reshape(B * S, *Ur.shape[2:]))
    shared = T.max_violation(q).reshape(B, S)
    np.testing.assert_array_equal(r.status, 0)
    np.testing.assert_allclose(r.c_max, cr, rtol=1e-9, atol=1e-12)
    assert (np.abs(cr - shared) > 1e-6).mean() > 0.5      # the shared bound would report something else for most samples


def test_guard_mode(hip, monkeypatch):
    """One small solve of the double-integrator fleet with red zones around every device array (the limits' array included) ends clean."""
    monkeypatch.setenv("TRAJOPT_GUARD", "1")
    s = F.spec("dint", 40)
    p = s.batch(hip)
    st = T.ALTROSolver(p).solve()
    assert (st.stats["status"] == F.OK).mean() > 0.9
    T.max_violation(p); T.evaluate_constraints(p, 0)
    T.clear_constraint_limits_batch(p)
    T.iLQRSolver(p, iterations=3).solve()
