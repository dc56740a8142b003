"""Per-trajectory cost weights on the MI355X (to_set_cost_weights_batch): one handle whose trajectories each have their own
diagonal Q / R, against B single-trajectory ORACLE problems built with trajectory b's weights (tests/cost_weight_fleets.py; vetted on the
oracle alone by tests/test_cost_weight_fleets_oracle.py).

Tolerances.  Phases: values at rtol 1e-11 (tests/test_gpu_constraint_limits.py::test_phases), with an absolute floor of 1e-12 times the
largest entry of the compared array — the entries of a cost block or a gradient are sums of products up to that size, so their rounding
differs by a few 1e-16 of it between two correct implementations, and an entry that cancels to nearly zero has no relative error to speak
of —, gains rtol 1e-6 / atol 1e-8, line-search indices equal, J of the forward pass rtol 1e-9.  Solves: integers (iterations,
iterations_outer, iterations_pn, status) bit-exact; cost, X, U at 1e-5 for AL and 1e-6 for ALTRO (test_gpu_constraint_limits.py::
test_solves) and 1e-6 for iLQR, 1e-4 for the trajectories the oracle itself cut off at an iteration limit (the per-trajectory-goal test of
tests/test_goal_batch.py); c_max rtol 1e-3 / atol 1e-9 (assert_solve_parity).

Observed on an MI355X: every solve's X / U within 2.1e-11 of the singles (the Quadrotor's iLQR solves; every other fleet below 1e-11), costs
within 1.5e-13, the policy rollout's J within 5.5e-14."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import cost_weight_fleets as F

pytestmark = pytest.mark.gpu

FLEETS = [("cartpole", 70, None), ("cartpole", 300, "lane"), ("dint", 40, None), ("quadrotor", 24, None), ("cartpole_knots", 70, None)]
IDS = [f"{n}-{B}" + (f"-{e}" if e else "") for n, B, e in FLEETS]
INTEGERS = ("iterations", "iterations_outer", "iterations_pn", "status")


def _env(monkeypatch, env):
    if env == "lane":  # the lane path with compaction, as tests/test_gpu_constraint_limits.py runs it
        monkeypatch.setenv("TRAJOPT_BACKWARD", "lane"); monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_MIN", "1")


def _path(p):
    info = np.zeros(8, dtype=np.int32)
    p._call("solver_path", p._pi(info))
    return list(info)


def _bits(p, s):
    return (T.states(p), T.controls(p)) + tuple(s.stats[k].copy() for k in INTEGERS + ("cost", "c_max"))


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y, err_msg=what)


def _close(a, ref, rtol, what):
    ref = np.asarray(ref)
    np.testing.assert_allclose(a, ref, rtol=rtol, atol=1e-12 * max(1.0, np.abs(ref).max()), err_msg=what)


def assert_fleet_solve(sh, ph, ref, rtol, unconverged_rtol=None, sel=None):
    """assert_solve_parity (tests/test_gpu_parity.py) with the stacked singles in the oracle batch's place, iterations_pn included."""
    from test_gpu_parity import assert_trajectories_close
    sel = np.arange(ph.B) if sel is None else np.asarray(sel)
    for k in INTEGERS:
        np.testing.assert_array_equal(sh.stats[k][sel], ref.stats[k], err_msg=k)
    done = (ref.stats["status"] == F.OK) if unconverged_rtol else np.ones(len(sel), bool)
    tol = np.where(done, rtol, unconverged_rtol or rtol)
    assert np.all(np.abs(sh.stats["cost"][sel] - ref.stats["cost"]) <= tol * np.abs(ref.stats["cost"])), "cost"
    np.testing.assert_allclose(sh.stats["c_max"][sel], ref.stats["c_max"], rtol=1e-3, atol=1e-9)
    assert_trajectories_close(T.states(ph)[sel], ref.X, tol, "X")
    assert_trajectories_close(T.controls(ph)[sel], ref.U, tol, "U")


# ------------------------------------------------------------------------------------------------ 1. phases
@pytest.mark.parametrize("variant", ["free", "bound"])
@pytest.mark.parametrize("name,B,env", FLEETS, ids=IDS)
def test_phases(name, B, env, variant, hip, oracle, monkeypatch):
    _env(monkeypatch, env)
    s = F.spec(name, B)
    ref = F.reference_phases(name, B, variant, oracle)
    ph = s.batch(hip, variant)
    r = F.phases(ph)
    _close(r.J, ref.J, 1e-11, "to_cost"); _close(r.Jk, ref.Jk, 1e-11, "to_stage_costs"); _close(r.al, ref.al, 1e-11, "to_al_cost")
    _close(r.grad, ref.grad, 1e-11, "to_cost_expansion gradient"); _close(r.hess, ref.hess, 1e-11, "to_cost_expansion Hessian")
    _close(r.E, ref.E, 1e-11, "to_get_cost_expansion")
    np.testing.assert_allclose(r.K, ref.K, rtol=1e-6, atol=1e-8); np.testing.assert_allclose(r.d, ref.d, rtol=1e-6, atol=1e-8)
    np.testing.assert_array_equal(r.ls, ref.ls); np.testing.assert_allclose(r.Jn, ref.Jn, rtol=1e-9)
    # the weights matter at this point: the handle on the shared nominal weights gives visibly different values
    shared = s.shared(hip, variant)
    rs = F.phases(shared)
    assert np.median(np.abs(rs.J - ref.J) / np.abs(ref.J)) > 1e-2
    assert np.abs(rs.hess - ref.hess).max() > 1e-2 * np.abs(ref.hess).max() and np.abs(rs.E - ref.E).max() > 1e-2 * np.abs(ref.E).max()
    assert np.abs(rs.K - ref.K).max() > 1e-3 * np.abs(ref.K).max()


# ------------------------------------------------------------------------------------------------ 2. solves
@pytest.mark.parametrize("solver", ["ilqr", "al", "altro"])
@pytest.mark.parametrize("name,B,env", FLEETS, ids=IDS)
def test_solves(name, B, env, solver, hip, oracle, monkeypatch):
    _env(monkeypatch, env)
    s = F.spec(name, B)
    ref = F.reference_solve(name, B, solver, oracle)
    Solver, kw = F.SOLVERS[solver]
    ph = s.batch(hip, F.variant_of(solver))
    path = _path(ph)
    assert path[5] == 0 and (env != "lane" or (path[0] == 2 and path[2] == 1))      # no scan kernel; lane: the lane layout with compaction
    sh = Solver(ph, **kw).solve()
    dev = np.maximum(F.relerr(T.states(ph), ref.X), F.relerr(T.controls(ph), ref.U))
    print(f"\n{name} B={B} {solver}: X / U deviate by <= {dev.max():.2e} (trajectory {dev.argmax()}), cost by <= "
          f"{(np.abs(sh.stats['cost'] - ref.stats['cost']) / np.abs(ref.stats['cost'])).max():.2e}")
    assert_fleet_solve(sh, ph, ref, F.solve_rtol(name, B, solver), unconverged_rtol=1e-4 if solver == "ilqr" else None)
    assert (sh.stats["status"] == F.OK).mean() >= 0.9


# ------------------------------------------------------------------------------------------------ 3. setter semantics
def test_setter_semantics(hip):
    s = F.spec("cartpole", 70)
    B = s.B
    p = s.shared(hip, "bound")
    Qn, Rn = s._nominal_weights()
    for ci in range(2):   # nothing set: the descriptor's diagonal, repeated
        Q, R = T.get_cost_weights_batch(p, ci)
        np.testing.assert_array_equal(Q, np.tile(Qn[ci], (B, 1))); np.testing.assert_array_equal(R, np.tile(Rn[ci], (B, 1)))
    fresh_path = _path(p)
    fresh = _bits(p, T.ALSolver(p, **F.AL_KW).solve())
    X0, U0 = T.states(p), T.controls(p)
    # set then get: the same bits; the setter leaves X, U alone; a NULL block stays as it is
    T.set_cost_weights_batch(p, 0, Q=s.Q[:, 0])
    np.testing.assert_array_equal(T.states(p), X0); np.testing.assert_array_equal(T.controls(p), U0)
    Q, R = T.get_cost_weights_batch(p, 0)
    np.testing.assert_array_equal(Q, s.Q[:, 0]); np.testing.assert_array_equal(R, np.tile(Rn[0], (B, 1)))
    T.set_cost_weights_batch(p, 0, R=s.R[:, 0])
    Q, R = T.get_cost_weights_batch(p, 0)
    np.testing.assert_array_equal(Q, s.Q[:, 0]); np.testing.assert_array_equal(R, s.R[:, 0])
    Q1, R1 = T.get_cost_weights_batch(p, 1)                                              # the other cost: still its descriptor's
    np.testing.assert_array_equal(Q1, np.tile(Qn[1], (B, 1))); np.testing.assert_array_equal(R1, np.tile(Rn[1], (B, 1)))
    assert _path(p)[1] == 0 and _path(p)[5] == 0                                         # flagged: no fused cooperative kernel, no scan kernel
    T.initial_controls(p, np.full(1, 0.01)); T.rollout(p)
    first = _bits(p, T.ALSolver(p, **F.AL_KW).solve())
    assert not np.array_equal(first[1], fresh[1])
    # to_set_cost restarts THAT cost's rows from the new descriptor, and only those
    T.set_cost_weights_batch(p, 1, Q=s.Q[:, 1], R=s.R[:, 1])
    c0 = p._cost_objs[0]
    new = T.DiagonalCost(2.0 * c0.Q, 3.0 * c0.R, c0.q, c0.r, c0.c)
    d = new._desc()
    p._call("set_cost", 0, T.capi.C.byref(d))
    Q, R = T.get_cost_weights_batch(p, 0)
    np.testing.assert_array_equal(Q, np.tile(2.0 * c0.Q, (B, 1))); np.testing.assert_array_equal(R, np.tile(3.0 * c0.R, (B, 1)))
    Q1, R1 = T.get_cost_weights_batch(p, 1)
    np.testing.assert_array_equal(Q1, s.Q[:, 1]); np.testing.assert_array_equal(R1, s.R[:, 1])
    d = c0._desc()
    p._call("set_cost", 0, T.capi.C.byref(d))
    # to_clear_...: every cost on its descriptor, the kernel variants of a fresh handle, its bits
    T.clear_cost_weights_batch(p)
    for ci in range(2):
        Q, R = T.get_cost_weights_batch(p, ci)
        np.testing.assert_array_equal(Q, np.tile(Qn[ci], (B, 1))); np.testing.assert_array_equal(R, np.tile(Rn[ci], (B, 1)))
    assert _path(p) == fresh_path
    T.initial_controls(p, np.full(1, 0.01)); T.rollout(p)
    _same_bits(_bits(p, T.ALSolver(p, **F.AL_KW).solve()), fresh, "after to_clear_cost_weights_batch")


@pytest.mark.parametrize("name,B,solver", [("cartpole", 70, "ilqr"), ("cartpole", 70, "altro"), ("quadrotor", 24, "ilqr")])
def test_weights_equal_to_the_descriptors_give_the_shared_handles_integers(name, B, solver, hip):
    s = F.spec(name, B)
    Solver, kw = F.SOLVERS[solver]
    shared = s.shared(hip, F.variant_of(solver))
    ss = Solver(shared, **kw).solve()
    p = s.shared(hip, F.variant_of(solver))
    Qn, Rn = s._nominal_weights()
    for ci in range(s.n_costs):
        T.set_cost_weights_batch(p, ci, Q=np.tile(Qn[ci], (B, 1)), R=np.tile(Rn[ci], (B, 1)))
    sp = Solver(p, **kw).solve()
    for k in INTEGERS:
        np.testing.assert_array_equal(sp.stats[k], ss.stats[k], err_msg=k)
    np.testing.assert_allclose(sp.stats["cost"], ss.stats["cost"], rtol=1e-9)
    assert np.maximum(F.relerr(T.states(p), T.states(shared)), F.relerr(T.controls(p), T.controls(shared))).max() < 1e-7


def test_refusals(hip):
    from trajectoryoptimization_jl_amd import configs
    B = 3
    p = configs.cartpole_problem(batch=B, N=11, tf=0.5, lib=hip)
    Q, R = np.ones((B, 4)), np.ones((B, 1))
    for bad in (-1, 2):
        with pytest.raises(T.ArgumentError, match="cost id out of range"):
            T.set_cost_weights_batch(p, bad, Q=Q)
        with pytest.raises(T.ArgumentError, match="cost id out of range"):
            T.get_cost_weights_batch(p, bad)
    with pytest.raises(T.ArgumentError, match="Q and R are both NULL"):
        p._call("set_cost_weights_batch", 0, None, None)
    Qb = Q.copy(); Qb[1, 2] = np.nan; Qb[2, 0] = np.inf
    with pytest.raises(T.ArgumentError, match=r"Q\[2\] of trajectory 1 is not finite"):
        T.set_cost_weights_batch(p, 0, Q=Qb, R=R)
    Rb = R.copy(); Rb[2, 0] = -np.inf
    with pytest.raises(T.ArgumentError, match=r"R\[0\] of trajectory 2 is not finite"):
        T.set_cost_weights_batch(p, 0, Q=Q, R=Rb)
    Qg, Rg = T.get_cost_weights_batch(p, 0)                                 # a refused call changes nothing
    np.testing.assert_array_equal(Qg, np.full((B, 4), 1e-2)); np.testing.assert_array_equal(Rg, np.full((B, 1), 1e-1))
    assert _path(p) == _path(configs.cartpole_problem(batch=B, N=11, tf=0.5, lib=hip))
    T.set_cost_weights_batch(p, 0, Q=-Q, R=0 * R)                           # no definiteness check: the descriptors get none either
    T.clear_cost_weights_batch(p)
    # dense kinds, by name
    obj = T.LQRObjective(np.eye(4) + 0.1, np.eye(1), np.eye(4), np.zeros(4), 11)
    pq = T.Problem(T.Cartpole(), obj, np.zeros(4), 0.5, batch=B, lib=hip)
    with pytest.raises(T.UnsupportedError, match="cost 0 is of kind QuadraticCost"):
        T.set_cost_weights_batch(pq, 0, Q=Q)
    quad = T.Quadrotor()
    xq = np.r_[0, 0, 0, 1.0, np.zeros(9)]
    eq = T.ErrorQuadratic(quad, np.ones(12), np.ones(4), xq)
    pe = T.Problem(quad, T.Objective(eq, 11), xq, 0.5, batch=B, lib=hip)
    with pytest.raises(T.UnsupportedError, match="cost 0 is of kind ErrorQuadratic"):
        T.set_cost_weights_batch(pe, 0, Q=np.ones((B, 13)), R=np.ones((B, 4)))
    # a stored tracking reference, in either order
    N = 11
    Xr, Ur = np.zeros((4, N)), np.zeros((1, N))
    pt = T.Problem(T.Cartpole(), T.TrackingObjective(np.ones(4), np.ones(1), Xr, Ur), np.zeros(4), 0.5, batch=B, lib=hip)
    T.set_tracking_reference_batch(pt, np.zeros((B, N, 4)))
    with pytest.raises(T.UnsupportedError, match="holds a tracking reference"):
        T.set_cost_weights_batch(pt, 0, Q=Q)
    T.clear_tracking_reference_batch(pt)
    T.set_cost_weights_batch(pt, 0, Q=Q)
    with pytest.raises(T.UnsupportedError, match="carries per-trajectory cost weights"):
        T.set_tracking_reference_batch(pt, np.zeros((B, N, 4)))
    # a model without per-trajectory weights
    from test_hybrid_dims import hybrid_problem
    hy = hybrid_problem(hip, batch=B)[0]
    with pytest.raises(T.UnsupportedError, match="hybrid double integrator"):
        hy._call("set_cost_weights_batch", 0, hy._pd(np.ones((B, hy.n))), None)
    # solve in flight
    s = F.spec("cartpole", 70)
    big = s.shared(hip, "bound")
    solver = T.ALSolver(big, **F.AL_KW)
    solver.solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="asynchronous solve is in flight"):
            T.set_cost_weights_batch(big, 0, Q=s.Q[:, 0])
        with pytest.raises(T.ArgumentError, match="asynchronous solve is in flight"):
            T.clear_cost_weights_batch(big)
    finally:
        solver.wait()


# ------------------------------------------------------------------------------------------------ 4. combinations
@pytest.mark.parametrize("solver", ["al", "altro"])
def test_combination_with_goals_limits_plants_and_steps(solver, hip, oracle):
    """Weights, goals (to_set_cost_linear_batch), control bounds (to_set_constraint_limits_batch), plants and time steps, all per trajectory on
    one handle, against singles built with all five; another order of the setters gives the same bits."""
    ref = F.combo_reference(oracle, solver)
    Solver, kw = F.SOLVERS[solver]
    pa = F.combo_apply(F.combo_shared(hip))
    sa = Solver(pa, **kw).solve()
    assert_fleet_solve(sa, pa, ref, 1e-5 if solver == "al" else 1e-6)
    assert (sa.stats["status"] == F.OK).mean() >= 0.9
    pb = F.combo_apply(F.combo_shared(hip), order=("steps", "plants", "limits", "weights"))
    _same_bits(_bits(pa, sa), _bits(pb, Solver(pb, **kw).solve()), "order of the setters")
    # one family cleared: what stays is what a handle that never had it computes
    T.clear_cost_weights_batch(pa)
    pc = F.combo_apply(F.combo_shared(hip), order=("limits", "plants", "steps"))
    c = F.combo()
    for q in (pa, pc):   # (the goals' linear terms stay on pa: the same ones onto pc)
        for i, Qi in enumerate((c.Q, c.Qf)):
            q._call("set_cost_linear_batch", i, q._pd(np.ascontiguousarray(-Qi * c.Xf)), q._pd(np.zeros((F.COMBO_B, 1))))
        T.initial_controls(q, np.full(1, 0.01)); T.rollout(q)
    _same_bits(_bits(pa, Solver(pa, **kw).solve()), _bits(pc, Solver(pc, **kw).solve()), "weights cleared next to the other arrays")


# ------------------------------------------------------------------------------------------------ 5. policy rollout, MPC
def test_policy_rollout_J_uses_each_trajectorys_weights(hip, oracle):
    """to_policy_rollout with S = 3 on the Cartpole fleet after a solve: J of every sample equals the oracle's cost of the CPU restatement
    (tests/test_gpu_policy_rollout.py restate) on a problem built with the trajectory's own weights."""
    from test_gpu_policy_rollout import restate, sample_starts, RTOL
    B, S = 70, 3
    s = F.spec("cartpole", B)
    p = s.batch(hip, "bound")
    T.ALSolver(p, **F.AL_KW).solve()
    I.expand(p); I.backwardpass(p)
    g = I.gains(p)
    Xbar, Ubar = T.states(p), T.controls(p)
    X0s = sample_starts(p, Xbar, 0.05, S)
    r = T.policy_rollout(p, X0s, trajectories=True)
    Xr, Ur, _ = restate(oracle, p, Xbar, Ubar, g["K"], g["d"], X0s)
    Jr, Js = np.zeros((B, S)), np.zeros((B, S))
    for b in range(B):
        for out, (Q, R) in ((Jr, (s.Q[b], s.R[b])), (Js, s._nominal_weights())):
            q = s._problem(oracle, S, 0, Q, R, "bound")
            T.initial_states(q, Xr[b]); T.initial_controls(q, Ur[b])
            out[b] = T.cost(q)
    np.testing.assert_array_equal(r.status, 0)
    dev = np.abs(r.J - Jr) / np.maximum(1.0, np.abs(Jr))
    print(f"\npolicy rollout J deviates by <= {dev.max():.2e}")
    assert dev.max() <= RTOL
    assert np.median(np.abs(Js - Jr) / np.abs(Jr)) > 1e-2          # the shared weights would report something else


def test_mpc_advance_leaves_the_weights_alone(hip):
    s = F.spec("cartpole", 70)
    p = s.batch(hip, "bound")
    before = [T.get_cost_weights_batch(p, ci) for ci in range(2)]
    T.ALSolver(p, **F.AL_KW).solve()
    path = _path(p)
    r = T.mpc_advance(p, shift=2)
    assert np.all(r.status == 0)
    for ci in range(2):
        for a, b in zip(T.get_cost_weights_batch(p, ci), before[ci]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(before[ci][0], s.Q[:, ci])
    assert _path(p) == path
    # ... and the device array too: the cost of the shifted problem is that of singles with the trajectories' own weights
    J = T.cost(p)
    X, U = T.states(p), T.controls(p)
    from oracle_binding import load_oracle
    oracle = load_oracle()
    for b in (0, 37, 69):
        q = s.single(oracle, b, "bound")
        T.initial_states(q, X[b:b + 1]); T.initial_controls(q, U[b:b + 1])
        np.testing.assert_allclose(J[b], T.cost(q)[0], rtol=1e-11)


# ------------------------------------------------------------------------------------------------ 6. repack, guard, batch independence
def test_repacked_solve_is_the_unrepacked_solve(hip, monkeypatch):
    """One small-batch iLQR solve on the fused lane path with a working set that moves again and again (TRAJOPT_REPACK=1), the weights
    travelling with their trajectories: bit-equal to the solve that never moves."""
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane"); monkeypatch.setenv("TRAJOPT_REPACK_AT", "0.9")
    s = F.spec("cartpole", 300)
    out = []
    for repack in ("1", "0"):
        monkeypatch.setenv("TRAJOPT_REPACK", repack)
        p = s.batch(hip, "free")
        assert bool(_path(p)[7] & 2) == (repack == "1")
        out.append(_bits(p, T.iLQRSolver(p).solve()))
        if repack == "1":   # a second solve on the same handle re-uses the working set
            T.initial_controls(p, np.full(1, 0.01)); T.rollout(p)
            _same_bits(_bits(p, T.iLQRSolver(p).solve()), out[0], "second repacked solve")
    _same_bits(out[0], out[1], "repacked vs unrepacked")
    assert len(np.unique(out[0][2])) > 10       # iteration counts spread out: the set did shrink in steps


def test_guard_mode(hip, monkeypatch):
    """One small solve of the double-integrator fleet with red zones around every device array (the weights' array included) ends clean."""
    monkeypatch.setenv("TRAJOPT_GUARD", "1")
    s = F.spec("dint", 40)
    p = s.batch(hip, "bound")
    st = T.ALTROSolver(p).solve()
    assert (st.stats["status"] == F.OK).mean() > 0.9
    T.cost(p); T.stage_costs(p); I.cost_gradient_hessian(p)
    T.clear_cost_weights_batch(p)
    T.iLQRSolver(p, iterations=3).solve()


@pytest.mark.parametrize("solver", ["ilqr", "altro"])
def test_batch_independence(solver, hip, monkeypatch):
    """Trajectory b of the fleet is bit-identical whether it sits in the batch of 70 or, with the same weights, in a batch of 1 — both on
    the cooperative backward pass with two-wave forward workgroups, forced through the environment switches."""
    monkeypatch.setenv("TRAJOPT_BACKWARD", "coop"); monkeypatch.setenv("TRAJOPT_FWD2", "1")
    s = F.spec("cartpole", 70)
    Solver, kw = F.SOLVERS[solver]
    variant = F.variant_of(solver)
    p = s.batch(hip, variant)
    path = _path(p)
    full = _bits(p, Solver(p, **kw).solve())
    for b in (0, 5, 63, 64, 69):
        q = s.shared(hip, variant, batch=1, b_offset=b)
        s.set_weights(q, sel=[b])
        assert _path(q) == path
        one = _bits(q, Solver(q, **kw).solve())
        for x, y in zip(one, full):
            np.testing.assert_array_equal(x[0], y[b], err_msg=f"trajectory {b}")
