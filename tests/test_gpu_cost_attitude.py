"""Per-trajectory attitude references on the MI355X (to_set_cost_attitude_batch / to_set_tracking_attitude): one handle whose
trajectories each have their own q_ref in their DiagonalQuatCosts, against B single-trajectory ORACLE problems built with trajectory b's
q_ref (tests/attitude_fleets.py; vetted on the oracle alone by tests/test_attitude_fleets_oracle.py), and — for the tracking windows —
against a twin handle fed through the host recipe, bit for bit.

Tolerances: those of tests/test_gpu_cost_weights.py.  Phases at rtol 1e-11 with an absolute floor of 1e-12 times the largest entry of the
compared array, gains (and the trajectory the forward pass accepts with them) rtol 1e-6 / atol 1e-8, line-search indices equal, J of the
forward pass rtol 1e-9.  Solves: integers bit-exact; cost, X, U at 1e-6 for iLQR and ALTRO, 1e-5 for AL (1e-4 for trajectories the oracle
itself cut off at an iteration limit); c_max rtol 1e-3 / atol 1e-9."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import attitude_fleets as AF
from test_gpu_cost_weights import _path, _bits, _same_bits, _close, assert_fleet_solve

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _restart(p, uf):
    T.initial_controls(p, uf); T.rollout(p)


# ------------------------------------------------------------------------------------------------ 1. phases
@pytest.mark.parametrize("variant,roll", [("free", False), ("bound", False), ("bound", True)])
def test_phases(variant, roll, hip, oracle, monkeypatch):
    if roll:   # the re-roll of accepted candidates evaluates the cost again
        monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_MIN", "1")
    g = AF.goal(70)
    ref = AF.reference_phases(70, variant)
    ph = g.batch(hip, variant)
    r = AF.phases(ph)
    _close(r.J, ref.J, 1e-11, "to_cost"); _close(r.Jk, ref.Jk, 1e-11, "to_stage_costs"); _close(r.al, ref.al, 1e-11, "to_al_cost")
    _close(r.grad, ref.grad, 1e-11, "to_cost_expansion gradient"); _close(r.hess, ref.hess, 1e-11, "to_cost_expansion Hessian")
    _close(r.E, ref.E, 1e-11, "to_get_cost_expansion")
    np.testing.assert_allclose(r.K, ref.K, rtol=1e-6, atol=1e-8); np.testing.assert_allclose(r.d, ref.d, rtol=1e-6, atol=1e-8)
    np.testing.assert_array_equal(r.ls, ref.ls); np.testing.assert_allclose(r.Jn, ref.Jn, rtol=1e-9)
    np.testing.assert_allclose(r.X, ref.X, rtol=1e-6, atol=1e-8); np.testing.assert_allclose(r.U, ref.U, rtol=1e-6, atol=1e-8)
    print(f"\ngoal B=70 {variant} roll={roll}: J deviates by <= {(np.abs(r.J - ref.J) / np.abs(ref.J)).max():.2e}, the expansion by <= "
          f"{np.abs(r.E - ref.E).max() / np.abs(ref.E).max():.2e} of its largest entry, the forward pass's J by <= {(np.abs(r.Jn - ref.Jn) / np.abs(ref.Jn)).max():.2e}")
    # the attitude matters at this point: the same handle with the goal POSITIONS alone (every member on the shared attitude) differs visibly
    rs = AF.phases(g.batch(hip, variant, attitude=False))
    # (J: the attitude term is at most N w = 31 of a cost near 1e3, and the 31 knots of the hover rollout share one attitude, so two references
    # differ by a few tenths per knot — some 1e-3 of J; what is asked here is a difference seven orders above the comparison's tolerance.  The
    # quaternion rows of the gradient carry nothing but -+ w q_ref: they differ in full.)
    assert np.median(np.abs(rs.J - ref.J) / np.abs(ref.J)) > 1e-4
    assert np.abs(rs.grad[..., 3:7] - ref.grad[..., 3:7]).max() > 1e-2          # components of two unit quaternions a rotation apart
    assert np.abs(rs.E - ref.E).max() > 1e-8 * np.abs(ref.E).max()              # three orders above the comparison's tolerance
    # ... and where q_ref enters the EXPANSION: the rotational rows of the error-state gradient (-+ w G(q)'q_ref / 2-ish: components of a unit
    # quaternion a rotation of tens of degrees apart) and the rotational block of the error-state Hessian (the term -(q'g) I of the attitude
    # Jacobian, w = 1 times a dot product of unit quaternions) are compared and must tell the two references apart by more than 1e-2
    _close(r.qx_rot, ref.qx_rot, 1e-11, "rotational rows of qx"); _close(r.Qxx_rot, ref.Qxx_rot, 1e-11, "rotational block of Qxx")
    print(f"  shared attitude: qx rot differs by {np.abs(rs.qx_rot - ref.qx_rot).max():.2e}, Qxx rot by {np.abs(rs.Qxx_rot - ref.Qxx_rot).max():.2e}, "
          f"d by {np.abs(rs.d - ref.d).max() / np.abs(ref.d).max():.2e} of its largest entry")
    assert np.abs(rs.qx_rot - ref.qx_rot).max() > 1e-2 and np.abs(rs.Qxx_rot - ref.Qxx_rot).max() > 1e-2
    assert np.abs(rs.d - ref.d).max() > 1e-3 * np.abs(ref.d).max()              # the gains: the bound of tests/test_gpu_cost_weights.py on K


# ------------------------------------------------------------------------------------------------ 2. solves
@pytest.mark.parametrize("solver", ["ilqr", "al", "altro"])
def test_solves(solver, hip, oracle):
    B = 24
    g = AF.goal(B)
    ref = AF.reference_solve("goal", B, solver)
    Solver, kw = AF.SOLVERS[solver]
    ph = g.batch(hip, AF.variant_of(solver))                    # T.set_goal_state(p, Xf, attitude=True)
    # routed and reported as a handle with weights
    pw = g.shared(hip, AF.variant_of(solver))
    for ci, (Q, R) in enumerate(((g.Q0, g.R0), (g.Qf0, g.R0))):
        T.set_cost_weights_batch(pw, ci, Q=np.tile(Q, (B, 1)), R=np.tile(R, (B, 1)))
    assert _path(ph) == _path(pw) and _path(ph)[5] == 0
    sh = Solver(ph, **kw).solve()
    dev = np.maximum(AF.relerr(T.states(ph), ref.X), AF.relerr(T.controls(ph), ref.U))
    print(f"\ngoal B={B} {solver}: X / U deviate by <= {dev.max():.2e} (trajectory {dev.argmax()}), cost by <= "
          f"{(np.abs(sh.stats['cost'] - ref.stats['cost']) / np.abs(ref.stats['cost'])).max():.2e}")
    assert_fleet_solve(sh, ph, ref, AF.solve_rtol("goal", B, solver), unconverged_rtol=1e-4 if solver == "ilqr" else None)
    assert (sh.stats["status"] == AF.OK).mean() >= 0.9


# ------------------------------------------------------------------------------------------------ 3. tracking twin
def _terms(p):
    return [T.get_cost_linear_batch(p, ci) + (T.get_cost_attitude_batch(p, ci),) for ci in range(len(p._cost_objs))]


def _same_terms(a, b, what):
    for ci, (x, y) in enumerate(zip(_terms(a), _terms(b))):
        for u, v in zip(x, y):
            assert same(u, v), f"{what}: cost {ci}"


@pytest.mark.parametrize("solver", ["ilqr", "altro"])
def test_tracking_twin(solver, hip):
    t = AF.tracking(70)
    Solver, kw = AF.SOLVERS[solver]
    v = AF.variant_of(solver)
    A, Bh = t.problem(hip, variant=v), t.problem(hip, variant=v)
    T.set_tracking_reference_batch(A, t.Xref, t.Uref, start=t.start, end="hold", attitude=True)
    assert T.get_tracking_attitude(A) and not T.get_tracking_attitude(Bh)
    t.feed_by_recipe(Bh, t.start)
    _same_terms(A, Bh, "first window")
    j = t.window(t.start, 4)
    assert same(T.get_cost_attitude_batch(A, int(A._cost_index[4])), t.Xref[np.arange(70), j, 3:7])     # exact copies of the right knot
    assert _path(A) == _path(Bh)
    _same_bits(_bits(A, Solver(A, **kw).solve()), _bits(Bh, Solver(Bh, **kw).solve()), "first window")
    T.set_tracking_window(A, t.start2)
    t.feed_by_recipe(Bh, t.start2)
    _same_terms(A, Bh, "second window")
    for p in (A, Bh):
        _restart(p, t.uf)
    sa = Solver(A, **kw).solve()
    _same_bits(_bits(A, sa), _bits(Bh, Solver(Bh, **kw).solve()), "second window")
    assert (sa.stats["status"] == AF.OK).mean() >= 0.9
    # a setter call between two window calls acts until the next window call; mode off: the tracked costs return to their descriptors
    q = np.tile([0.6, 0.0, 0.8, 0.0], (70, 1))
    T.set_cost_attitude_batch(A, 3, q)
    assert same(T.get_cost_attitude_batch(A, 3), q)
    T.set_tracking_window(A, t.start2)
    _same_terms(A, Bh, "window after a setter call")
    T.set_tracking_attitude(A, False)
    for ci in (0, 3, 20):
        assert same(T.get_cost_attitude_batch(A, ci), np.tile(AF.IDENTITY, (70, 1)))
    assert same(T.get_cost_linear_batch(A, 3)[0], T.get_cost_linear_batch(Bh, 3)[0])                      # the linear terms stay
    T.set_tracking_window(A, t.start)                                                                     # off: lowers what it always lowered
    assert same(T.get_cost_attitude_batch(A, 3), np.tile(AF.IDENTITY, (70, 1)))


@pytest.mark.parametrize("solver", ["ilqr", "altro"])
def test_tracking_against_the_oracle_singles(solver, hip, oracle):
    B = 24
    t = AF.tracking(B)
    ref = AF.reference_solve("tracking", B, solver)
    Solver, kw = AF.SOLVERS[solver]
    p = t.problem(hip, variant=AF.variant_of(solver))
    T.set_tracking_reference_batch(p, t.Xref, t.Uref, start=t.start, end="hold", attitude=True)
    sh = Solver(p, **kw).solve()
    dev = np.maximum(AF.relerr(T.states(p), ref.X), AF.relerr(T.controls(p), ref.U))
    print(f"\ntracking B={B} {solver}: X / U deviate by <= {dev.max():.2e} (trajectory {dev.argmax()})")
    assert_fleet_solve(sh, p, ref, AF.solve_rtol("tracking", B, solver), unconverged_rtol=1e-4 if solver == "ilqr" else None)
    assert (sh.stats["status"] == AF.OK).mean() >= 0.9


# ------------------------------------------------------------------------------------------------ 4. MPC
def test_mpc_run_moves_the_attitude_windows(hip):
    steps, s = 3, 2
    t = AF.tracking(70)
    B, Nref = t.B, t.Nref
    p, twin = t.problem(hip), t.problem(hip)
    start0 = (1 + np.arange(B) % 9).astype(np.int32)            # 1 .. 9: every window fits at first, the later ones pass the end within the run (held)
    T.set_tracking_reference_batch(p, t.Xref, t.Uref, start=start0, end="hold", attitude=True)
    x_true = t.x0.copy()
    rec = T.mpc_run(T.iLQRSolver(p, iterations=25), steps, shift=s, x_true=x_true, advance_reference=True)
    stwin, start = T.iLQRSolver(twin, iterations=25), start0.astype(np.int64)
    X_cl, U_cl = np.empty_like(rec.X_cl), np.empty_like(rec.U_cl)
    for k in range(steps):
        one = T.mpc_run(stwin, 1, shift=s, x_true=x_true if k == 0 else None, before_solve=lambda prob, _t: t.feed_by_recipe(prob, start))
        assert np.array_equal(rec.iterations[k], one.iterations[0]) and np.array_equal(rec.status[k], one.status[0]), k
        assert np.array_equal(rec.advance_status[k], one.advance_status[0]), k
        if k == 0:
            X_cl[:, 0] = one.X_cl[:, 0]
        X_cl[:, k * s + 1:(k + 1) * s + 1], U_cl[:, k * s:(k + 1) * s] = one.X_cl[:, 1:], one.U_cl
        start = np.minimum(start + np.where(one.advance_status[0] == 0, s, 0), Nref)
    assert same(rec.X_cl, X_cl) and same(rec.U_cl, U_cl)
    assert np.array_equal(T.get_tracking_window(p)[2], start) and (start - 1 + t.N > Nref).any()
    assert same(T.controls(p), T.controls(twin))
    jl = t.window(start, t.N - 1)                                 # the last window's attitude rows are on the device
    assert same(T.get_cost_attitude_batch(p, int(p._cost_index[t.N - 1])), t.Xref[np.arange(B), jl, 3:7])


# ------------------------------------------------------------------------------------------------ 5. setter semantics
def test_setter_semantics(hip):
    B = 24
    g = AF.goal(B)
    p = g.shared(hip, "bound")
    desc = np.tile(g.xf[3:7], (B, 1))
    for ci in range(2):   # nothing set: the descriptor's q_ref, repeated
        assert same(T.get_cost_attitude_batch(p, ci), desc)
    fresh_path = _path(p)
    fresh = _bits(p, T.ALSolver(p, **AF.F.AL_KW).solve())
    _restart(p, g.uf)
    X0, U0 = T.states(p), T.controls(p)
    A = np.ascontiguousarray(g.Xf[:, 3:7])
    T.set_cost_attitude_batch(p, 0, A)
    assert same(T.states(p), X0) and same(T.controls(p), U0)                 # the setter leaves X, U alone
    assert same(T.get_cost_attitude_batch(p, 0), A)                          # set then get: the same bits
    assert same(T.get_cost_attitude_batch(p, 1), desc)                       # the other cost keeps its descriptor's q_ref
    assert _path(p)[1] == 0 and _path(p)[5] == 0                               # flagged: no fused cooperative kernel, no scan kernel
    Q, R = T.get_cost_weights_batch(p, 0)                                    # gw rides along on the descriptors' diagonals
    assert same(Q, np.tile(g.Q0, (B, 1))) and same(R, np.tile(g.R0, (B, 1)))
    first = _bits(p, T.ALSolver(p, **AF.F.AL_KW).solve())
    assert not np.array_equal(first[1], fresh[1])
    # to_set_cost restarts THAT cost's rows from the new descriptor, and only those
    T.set_cost_attitude_batch(p, 1, -2.0 * A)                                # used as given: neither normalised nor sign-fixed
    c0 = p._cost_objs[0]
    new = T.DiagonalQuatCost(c0.Q, c0.R, c0.q, c0.r, c0.c, c0.w, [0.0, 1.0, 0.0, 0.0])
    d = new._desc()
    p._call("set_cost", 0, T.capi.C.byref(d))
    assert same(T.get_cost_attitude_batch(p, 0), np.tile([0.0, 1.0, 0.0, 0.0], (B, 1))) and same(T.get_cost_attitude_batch(p, 1), -2.0 * A)
    d = c0._desc()
    p._call("set_cost", 0, T.capi.C.byref(d))
    # weights next to attitudes: to_clear_cost_weights_batch keeps the routing and the attitudes, gw returns to the descriptors
    T.set_cost_weights_batch(p, 0, Q=np.tile(2.0 * g.Q0, (B, 1)))
    routed = _path(p)
    T.clear_cost_weights_batch(p)
    assert _path(p) == routed and same(T.get_cost_weights_batch(p, 0)[0], np.tile(g.Q0, (B, 1))) and same(T.get_cost_attitude_batch(p, 1), -2.0 * A)
    # to_clear_...: every cost on its descriptor, the kernel variants of a fresh handle, its bits
    T.clear_cost_attitude_batch(p)
    for ci in range(2):
        assert same(T.get_cost_attitude_batch(p, ci), desc)
    assert _path(p) == fresh_path
    _restart(p, g.uf)
    _same_bits(_bits(p, T.ALSolver(p, **AF.F.AL_KW).solve()), fresh, "after to_clear_cost_attitude_batch")
    # every call is refused while a solve is in flight
    solver = T.ALSolver(p, **AF.F.AL_KW)
    _restart(p, g.uf)
    solver.solve_async()
    try:
        for call in (lambda: T.set_cost_attitude_batch(p, 0, A), lambda: T.get_cost_attitude_batch(p, 0), lambda: T.clear_cost_attitude_batch(p),
                     lambda: T.set_tracking_attitude(p, True)):
            with pytest.raises(T.ArgumentError, match="asynchronous solve is in flight"):
                call()
    finally:
        solver.wait()


def test_refusals_and_the_weights_tracking_rules(hip):
    from trajectoryoptimization_jl_amd import configs
    B = 3
    t = AF.tracking(B)
    p = t.problem(hip)
    A = np.tile([0.6, 0.0, 0.0, 0.8], (B, 1))
    for bad in (-1, t.N):
        with pytest.raises(T.ArgumentError, match="cost id out of range"):
            T.set_cost_attitude_batch(p, bad, A)
    Ab = A.copy(); Ab[1, 2] = np.nan; Ab[2, 0] = np.inf
    with pytest.raises(T.ArgumentError, match=r"q_ref\[2\] of trajectory 1 is not finite"):
        T.set_cost_attitude_batch(p, 0, Ab)
    with pytest.raises(T.ArgumentError, match="no tracking reference is set"):
        T.set_tracking_attitude(p, True)
    fresh = _path(p)
    assert same(T.get_cost_attitude_batch(p, 0), np.tile(AF.IDENTITY, (B, 1))) and not T.get_tracking_attitude(p)   # a refused call changes nothing
    # a tracking reference is accepted on an attitude-only handle and refused once the CALLER sets weights
    T.set_cost_attitude_batch(p, 0, A)
    T.set_tracking_reference_batch(p, t.Xref, t.Uref, start=t.start, end="hold")
    with pytest.raises(T.UnsupportedError, match="holds a tracking reference"):
        T.set_cost_weights_batch(p, 0, Q=np.ones((B, 13)))
    assert same(T.get_cost_attitude_batch(p, 0), A)                           # attitude off: the window call left the setter's rows alone
    T.clear_tracking_reference_batch(p)
    T.set_cost_weights_batch(p, 0, Q=np.ones((B, 13)))
    with pytest.raises(T.UnsupportedError, match="carries per-trajectory cost weights"):
        T.set_tracking_reference_batch(p, t.Xref, t.Uref, start=t.start, end="hold")
    T.clear_cost_weights_batch(p)                                             # the attitudes stay, gw is back on the descriptors: accepted again
    T.set_tracking_reference_batch(p, t.Xref, t.Uref, start=t.start, end="hold", attitude=True)
    T.clear_tracking_reference_batch(p)                                       # ... turns the mode off and returns the tracked costs to their descriptors
    assert not T.get_tracking_attitude(p) and same(T.get_cost_attitude_batch(p, 5), np.tile(AF.IDENTITY, (B, 1)))
    T.clear_cost_attitude_batch(p)
    assert _path(p) == fresh
    # kinds and models
    c = configs.cartpole_problem(batch=B, N=11, tf=0.5, lib=hip)
    with pytest.raises(T.UnsupportedError, match="cost 0 is of kind DiagonalCost"):
        T.set_cost_attitude_batch(c, 0, A)
    with pytest.raises(T.ArgumentError, match="no DiagonalQuatCost"):
        T.set_goal_state(c, np.zeros((B, 4)), attitude=True)
    quad = T.Quadrotor()
    xq = np.r_[0, 0, 0, 1.0, np.zeros(9)]
    pe = T.Problem(quad, T.Objective(T.ErrorQuadratic(quad, np.ones(12), np.ones(4), xq), 11), xq, 0.5, batch=B, lib=hip)
    with pytest.raises(T.UnsupportedError, match="cost 0 is of kind ErrorQuadratic"):
        T.set_cost_attitude_batch(pe, 0, A)
    N = 11
    pt = T.Problem(T.Cartpole(), T.TrackingObjective(np.ones(4), np.ones(1), np.zeros((4, N)), np.zeros((1, N))), np.zeros(4), 0.5, batch=B, lib=hip)
    T.set_tracking_reference_batch(pt, np.zeros((B, N, 4)))
    with pytest.raises(T.UnsupportedError, match="none of the tracked costs is a DiagonalQuatCost"):
        T.set_tracking_attitude(pt, True)
    from test_hybrid_dims import hybrid_problem
    hy = hybrid_problem(hip, batch=B)[0]
    with pytest.raises(T.UnsupportedError, match="hybrid double integrator"):
        hy._call("set_cost_attitude_batch", 0, hy._pd(np.ones((B, 4))))


def test_combination_with_weights_goals_and_limits(hip, oracle):
    """Attitudes, caller weights, linear terms (the goals) and control limits, all per trajectory on one handle, against singles built with
    all four."""
    ref = AF.combo_reference("altro")
    p = AF.combo_batch(hip)
    s = T.ALTROSolver(p).solve()
    dev = np.maximum(AF.relerr(T.states(p), ref.X), AF.relerr(T.controls(p), ref.U))
    print(f"\ncombination altro: X / U deviate by <= {dev.max():.2e}")
    assert_fleet_solve(s, p, ref, 1e-6)
    assert (s.stats["status"] == AF.OK).mean() >= 0.9


# ------------------------------------------------------------------------------------------------ 6. policy rollout
def test_policy_rollout_J_uses_each_trajectorys_attitude(hip, oracle):
    from test_gpu_policy_rollout import restate, sample_starts, RTOL
    B, S = 24, 2
    g = AF.goal(B)
    p = g.batch(hip, "free")
    T.iLQRSolver(p).solve()
    I.expand(p); I.backwardpass(p)
    gn = I.gains(p)
    Xbar, Ubar = T.states(p), T.controls(p)
    X0s = sample_starts(p, Xbar, 0.05, S)
    r = T.policy_rollout(p, X0s, trajectories=True)
    Xr, Ur, _ = restate(oracle, p, Xbar, Ubar, gn["K"], gn["d"], X0s)
    Jr, Js = np.zeros((B, S)), np.zeros((B, S))
    for b in range(B):
        for out, qref in ((Jr, g.Xf[b, 3:7]), (Js, g.xf[3:7])):
            q = g._problem(oracle, S, 0, g.Xf[b], qref, "free")
            T.initial_states(q, Xr[b]); T.initial_controls(q, Ur[b])
            out[b] = T.cost(q)
    np.testing.assert_array_equal(r.status, 0)
    dev = np.abs(r.J - Jr) / np.maximum(1.0, np.abs(Jr))
    print(f"\npolicy rollout J deviates by <= {dev.max():.2e}")
    assert dev.max() <= RTOL
    assert np.median(np.abs(Js - Jr) / np.abs(Jr)) > 1e-2          # the shared attitude would report something else


# ------------------------------------------------------------------------------------------------ 7. guard
def test_guard_mode(hip, monkeypatch):
    """The tracking twin's first solve with red zones around every device array (the attitude array included) ends clean."""
    monkeypatch.setenv("TRAJOPT_GUARD", "1")
    t = AF.tracking(70)
    p = t.problem(hip)
    T.set_tracking_reference_batch(p, t.Xref, t.Uref, start=t.start, end="hold", attitude=True)
    st = T.iLQRSolver(p).solve()            # (a red zone written to ends a call with a HipError that names the array)
    assert (st.stats["status"] == AF.OK).mean() >= 0.9
    T.set_tracking_window(p, t.start2)
    T.set_cost_attitude_batch(p, 0, np.tile(AF.IDENTITY, (70, 1)))
    T.cost(p); T.stage_costs(p); I.cost_gradient_hessian(p)
    T.clear_tracking_reference_batch(p)
    T.clear_cost_attitude_batch(p)
    T.iLQRSolver(p, iterations=3).solve()
