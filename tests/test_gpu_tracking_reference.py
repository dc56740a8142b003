"""One tracking reference per trajectory, windowed on the device (to_set_tracking_reference_batch / to_set_tracking_window) on the MI355X.

The reference is always a TWIN handle driven through entry points that exist without the feature: N raw ``set_cost_linear_batch`` calls
with q_b = -Q x_ref[j], r_b = -R u_ref[j] computed in numpy by the element-wise / ascending-order expressions of the header
(tests/tracking_fleets.py ``feed_by_recipe``).  The kernel promises the bits of that recipe, so every twin comparison is equality of BITS
(``same``); no measured number enters a tolerance.  The fleets are vetted on the CPU oracle by tests/test_tracking_fleets_oracle.py; against
the B single-trajectory oracle problems the tolerance is the project's own: integers exact, cost / X / U within rtol = 1e-6 in the
per-trajectory max norm (tests/test_gpu_parity.py assert_solve_parity, restated in ``assert_oracle_parity``)."""
import ctypes as C

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import capi
import tracking_fleets as F

pytestmark = pytest.mark.gpu

RTOL = 1e-6
STATS = ("iterations", "iterations_outer", "status")


def same(a, b):
    """Equality of bits (a NaN equals the same NaN, -0.0 does not equal 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return bool(np.array_equal(a, b))


def assert_same_terms(p, twin, what):
    for cid in range(len(p._cost_objs)):
        (q, r), (qt, rt) = T.get_cost_linear_batch(p, cid), T.get_cost_linear_batch(twin, cid)
        assert same(q, qt), f"{what}: q of cost {cid} differs in {int((q != qt).sum())} entries"
        assert same(r, rt), f"{what}: r of cost {cid} differs in {int((r != rt).sum())} entries"


def solve_both(p, twin, fleet, what, solver=T.iLQRSolver, **kw):
    out = []
    for q in (p, twin):
        s = solver(q, **{**fleet.solver_kw, **kw}).solve()
        out.append((s, T.states(q), T.controls(q)))
    (s, X, U), (st, Xt, Ut) = out
    for k in STATS:
        assert np.array_equal(s.stats[k], st.stats[k]), f"{what}: {k}"
    assert same(X, Xt) and same(U, Ut) and same(s.stats["cost"], st.stats["cost"]), what
    return s, X, U


def assert_oracle_parity(s, X, U, ref):
    """assert_solve_parity's measure against the stacked single-trajectory oracle solves."""
    for k in F.INT_STATS:
        np.testing.assert_array_equal(s.stats[k], ref[k], err_msg=k)
    np.testing.assert_allclose(s.stats["cost"], ref["cost"], rtol=RTOL)
    for A, R, name in ((X, ref["X"], "X"), (U, ref["U"], "U")):
        err = np.abs(A - R).reshape(len(R), -1).max(axis=1)
        scale = np.maximum(1.0, np.abs(R).reshape(len(R), -1).max(axis=1))
        assert np.all(err <= RTOL * scale), (name, int(np.argmax(err / scale)), float((err / scale).max()))


def pair(fleet, hip, end="refuse", start=None, with_u=True, **kw):
    """(feature handle, twin) of a fleet: one call against N calls."""
    start = fleet.start if start is None else start
    p, twin = fleet.problem(hip, **kw), fleet.problem(hip, **kw)
    T.set_tracking_reference_batch(p, fleet.Xref, fleet.Uref if with_u else None, start, end=end)
    F.feed_by_recipe(twin, fleet.Xref, fleet.Uref if with_u else None, start)
    return p, twin


# ------------------------------------------------------------------------------------------------ 4. twin against feature handle, 5. oracle
@pytest.mark.parametrize("name", sorted(F.FLEETS))
def test_one_call_equals_the_host_recipe_and_the_oracle(name, hip):
    fleet = F.FLEETS[name]()
    p, twin = pair(fleet, hip)
    assert_same_terms(p, twin, name)
    q0, r0 = T.get_cost_linear_batch(p, int(p._cost_index[0]))
    assert np.ptp(q0, axis=0).max() > 0 and np.ptp(r0, axis=0).max() > 0, "the terms differ from trajectory to trajectory"
    Nref, end, start = T.get_tracking_window(p)
    assert (Nref, end) == (fleet.Nref, "refuse") and np.array_equal(start, fleet.start) and start.dtype == np.int32
    s, X, U = solve_both(p, twin, fleet, name)
    assert_oracle_parity(s, X, U, F.oracle_singles(name))


def test_constrained_cartpole_fleet_under_the_al_solver(hip):
    fleet = F.cartpole_fleet()
    p, twin = pair(fleet, hip, constrained=True)
    assert_same_terms(p, twin, "constrained")
    s, X, U = solve_both(p, twin, fleet, "constrained cartpole, AL", solver=T.ALSolver)
    assert np.all(s.stats["iterations_outer"] >= 1)


# ------------------------------------------------------------------------------------------------ 6. window moves
def test_window_moves_equal_a_twin_fed_again(hip):
    fleet = F.cartpole_fleet()
    p, twin = pair(fleet, hip, end="hold")
    b = np.arange(fleet.B)
    moves = [(1 + (5 * b) % 17).astype(np.int32),                              # starts that differ inside one 64-lane tile
             np.where(b % 3 == 0, fleet.Nref - 4, 2 + b % 11).astype(np.int32),  # a third of the windows run past the end: held at the last knot
             np.full(fleet.B, fleet.Nref, np.int32)]                           # every knot of every trajectory on the last reference knot
    for i, start in enumerate(moves):
        T.set_tracking_window(p, start)
        F.feed_by_recipe(twin, fleet.Xref, fleet.Uref, start)
        assert_same_terms(p, twin, f"move {i}")
        Nref, end, got = T.get_tracking_window(p)
        assert (Nref, end) == (fleet.Nref, "hold") and np.array_equal(got, start)
        T.initial_controls(p, fleet.U0); T.initial_controls(twin, fleet.U0)
        solve_both(p, twin, fleet, f"move {i}")
    # refuse: the library's own refusal (raw call), and nothing changed
    q, _ = pair(fleet, hip, end="refuse")
    bad = fleet.start.copy()
    bad[66] = fleet.Nref - fleet.N + 2
    with pytest.raises(T.ArgumentError, match="reference trajectory too short for trajectory 66"):
        T.set_tracking_window(q, bad)
    assert np.array_equal(T.get_tracking_window(q)[2], fleet.start)
    with pytest.raises(T.ArgumentError, match="start of trajectory 0 is 0"):
        T.set_tracking_window(q, np.zeros(fleet.B, np.int32))
    with pytest.raises(ValueError, match="start is NULL"):
        q._call("set_tracking_window", None)
    fresh = fleet.problem(hip)
    with pytest.raises(T.ArgumentError, match="no tracking reference is set"):
        T.set_tracking_window(fresh, 1)
    assert T.get_tracking_window(fresh)[0] == 0
    shared = T.Problem(fleet.model, T.LQRObjective(np.ones(4), np.ones(1), np.ones(4), np.zeros(4), fleet.N), np.zeros(4), fleet.tf, batch=fleet.B, lib=hip)
    with pytest.raises(T.ArgumentError, match=r"needs a tracking objective \(a distinct cost per knot\)"):
        T.set_tracking_reference_batch(shared, fleet.Xref)
    Xbad = fleet.Xref.copy()
    Xbad[5, 7, 1] = np.nan
    with pytest.raises(T.ArgumentError, match="trajectory 5 is not finite at knot 8"):
        T.set_tracking_reference_batch(fresh, Xbad)
    assert T.get_tracking_window(fresh)[0] == 0


# ------------------------------------------------------------------------------------------------ 7. interactions
def test_without_controls_an_r_set_earlier_stays(hip):
    fleet = F.cartpole_fleet()
    p, twin = fleet.problem(hip), fleet.problem(hip)
    r_own = np.ascontiguousarray(0.01 * np.arange(fleet.B, dtype=np.float64)[:, None] + 0.5)
    cid = int(p._cost_index[3])
    for q in (p, twin):
        q._call("set_cost_linear_batch", cid, None, q._pd(r_own))
    T.set_tracking_reference_batch(p, fleet.Xref, None, fleet.start)
    F.feed_by_recipe(twin, fleet.Xref, None, fleet.start)
    assert_same_terms(p, twin, "Uref=None")
    assert same(T.get_cost_linear_batch(p, cid)[1], (p._cost_objs[cid].r[None, :] + (r_own - p._cost_objs[cid].r[None, :])))
    solve_both(p, twin, fleet, "Uref=None")


def test_set_cost_then_a_window_call_lowers_from_the_new_descriptor(hip):
    fleet = F.cartpole_fleet()
    p, twin = pair(fleet, hip)
    k = 6
    cid = int(p._cost_index[k])
    for q in (p, twin):
        c = q._cost_objs[cid]
        c.Q, c.q = c.Q * np.array([2.0, 0.5, 1.5, 3.0]), c.q + 0.125
        d = c._desc()
        q._call("set_cost", cid, C.byref(d))
    q_after, _ = T.get_cost_linear_batch(p, cid)
    assert same(q_after, np.tile(p._cost_objs[cid].q, (fleet.B, 1))), "to_set_cost starts the cost over"
    T.set_tracking_window(p, fleet.start)
    F.feed_by_recipe(twin, fleet.Xref, fleet.Uref, fleet.start)
    assert_same_terms(p, twin, "after set_cost and a window call")
    solve_both(p, twin, fleet, "after set_cost and a window call")


def test_clear_cost_linear_batch_keeps_the_reference(hip):
    fleet = F.cartpole_fleet()
    p, twin = pair(fleet, hip)
    T.clear_goal_state_batch(p)
    cid = int(p._cost_index[2])
    assert np.array_equal(T.get_cost_linear_batch(p, cid)[0], np.tile(p._cost_objs[cid].q, (fleet.B, 1)))   # (values: c.q + 0.0 loses the sign of a -0.0)
    assert T.get_tracking_window(p)[0] == fleet.Nref
    T.set_tracking_window(p, fleet.start)
    assert_same_terms(p, twin, "restored")
    solve_both(p, twin, fleet, "restored")


def test_clear_tracking_reference_then_a_fresh_handle(hip):
    fleet = F.cartpole_fleet()
    p, _ = pair(fleet, hip)
    T.iLQRSolver(p, **fleet.solver_kw).solve()
    T.clear_tracking_reference_batch(p)
    assert T.get_tracking_window(p)[0] == 0
    fresh = fleet.problem(hip)
    p.set_initial_state(fleet.x0); T.initial_controls(p, fleet.U0)
    from test_handle_reuse_oracle import solver_path
    assert np.array_equal(solver_path(p), solver_path(fresh))
    solve_both(p, fresh, fleet, "cleared against fresh")


def test_next_to_plants_time_steps_and_bounds(hip):
    import model_params_fleet as M
    import time_step_fleets as S
    fleet = F.cartpole_fleet()
    B = fleet.B
    models = M.draw_models("cartpole", B, 31)
    steps = S.draw_steps(fleet.tf, fleet.N, B, 32, ragged=True)
    up = (4.0 + 0.02 * np.arange(B))[:, None]
    p, twin = pair(fleet, hip, constrained=True)
    for q in (p, twin):
        T.set_model_params(q, models)
        T.set_time_steps_batch(q, steps)
        T.set_bounds_batch(q, 0, u_max=up, u_min=-up)
    T.set_tracking_window(p, fleet.start)           # (a window call after the other per-trajectory arrays appeared)
    assert_same_terms(p, twin, "combination")
    solve_both(p, twin, fleet, "combination", solver=T.ALSolver)


# ------------------------------------------------------------------------------------------------ 8. path coverage
def test_repacked_working_set_carries_the_terms(hip, monkeypatch):
    from test_handle_reuse_oracle import solver_path
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")
    monkeypatch.setenv("TRAJOPT_REPACK_AT", "0.9")
    monkeypatch.setenv("TRAJOPT_GUARD", "0")
    fleet = F.cartpole_fleet(B=200)
    out = []
    for repack in ("1", "0"):
        monkeypatch.setenv("TRAJOPT_REPACK", repack)
        p = fleet.problem(hip)
        T.set_tracking_reference_batch(p, fleet.Xref, fleet.Uref, fleet.start)
        path = solver_path(p)
        assert bool(path[7] & 2) == (repack == "1"), path
        s = T.iLQRSolver(p, **fleet.solver_kw).solve()
        out.append((s, T.states(p), T.controls(p), [T.get_cost_linear_batch(p, c) for c in range(fleet.N)]))
    (s1, X1, U1, g1), (s0, X0, U0, g0) = out
    it = s1.stats["iterations"]
    active = np.array([(it > k).sum() for k in range(int(it.max()) + 1)])
    assert ((active > 1) & (active < 0.9 * fleet.B)).any(), ("the batch must drain unevenly for a move to happen", active)
    for k in STATS:
        assert np.array_equal(s1.stats[k], s0.stats[k]), k
    assert same(X1, X0) and same(U1, U0) and same(s1.stats["cost"], s0.stats["cost"])
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(g1, g0)), "the home array after the solve"


def test_runs_clean_under_the_guard(hip, monkeypatch):
    fleet = F.cartpole_fleet()
    out = []
    for guard in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_GUARD", guard)               # read at to_create
        p = fleet.problem(hip)
        T.set_tracking_reference_batch(p, fleet.Xref, fleet.Uref, fleet.start, end="hold")
        T.set_tracking_window(p, np.full(fleet.B, fleet.Nref, np.int32))
        T.set_tracking_window(p, fleet.start)
        s = T.iLQRSolver(p, **fleet.solver_kw).solve()          # (a red zone written to ends a call with a HipError that names the array)
        out.append((T.states(p), T.controls(p), s.stats["iterations"].copy(), T.get_cost_linear_batch(p, 0)))
        T.clear_tracking_reference_batch(p)
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]) and same(out[0][3][0], out[1][3][0])


# ------------------------------------------------------------------------------------------------ 9. the closed loop
def test_mpc_run_moves_the_windows_on_the_device(hip):
    steps, s, limit = 4, 2, 1e2
    fleet = F.cartpole_fleet(Nref=60)
    B, Nref = fleet.B, fleet.Nref
    kw = dict(options=T.SolverOptions(lib=hip, max_state_value=limit))
    p, twin = fleet.problem(hip, **kw), fleet.problem(hip, **kw)
    start0 = (Nref - fleet.N - 6 + np.arange(B) % 7).astype(np.int32)   # 33 .. 39: every window fits at first, some pass the end within the run (held)
    x_true = fleet.x0.copy()
    x_true[:, 0] = 0.01 * np.arange(B)
    x_true[5, 0] = 10 * limit                                      # trajectory 5 arrives beyond max_state_value in the first period: a reported status
    T.set_tracking_reference_batch(p, fleet.Xref, fleet.Uref, start0, end="hold")
    rec = T.mpc_run(T.iLQRSolver(p, **fleet.solver_kw), steps, shift=s, x_true=x_true)
    # the twin: today's loop, one period at a time, the host recipe in the before_solve hook with the same bookkeeping of the starts
    stwin, start = T.iLQRSolver(twin, **fleet.solver_kw), start0.astype(np.int64)
    X_cl, U_cl = np.empty_like(rec.X_cl), np.empty_like(rec.U_cl)
    starts_seen = []
    for t in range(steps):
        starts_seen.append(start.copy())
        one = T.mpc_run(stwin, 1, shift=s, x_true=x_true if t == 0 else None,
                        before_solve=lambda prob, _t: F.feed_by_recipe(prob, fleet.Xref, fleet.Uref, start))
        assert np.array_equal(rec.iterations[t], one.iterations[0]) and np.array_equal(rec.status[t], one.status[0]), t
        assert np.array_equal(rec.advance_status[t], one.advance_status[0]) and np.array_equal(rec.k_limit[t], one.k_limit[0]), t
        if t == 0:
            X_cl[:, 0] = one.X_cl[:, 0]
        X_cl[:, t * s + 1:(t + 1) * s + 1], U_cl[:, t * s:(t + 1) * s] = one.X_cl[:, 1:], one.U_cl
        start = np.minimum(start + np.where(one.advance_status[0] == 0, s, 0), Nref)
    assert same(rec.X_cl, X_cl) and same(rec.U_cl, U_cl)
    assert rec.advance_status[0, 5] == capi.STATE_LIMIT and np.count_nonzero(rec.advance_status) == 1
    got = T.get_tracking_window(p)[2]
    assert np.array_equal(got, start) and got[5] == start0[5] + s * (steps - 1) and got[4] == min(start0[4] + s * steps, Nref)
    assert (starts_seen[-1] - 1 + fleet.N > Nref).any() and (starts_seen[0] - 1 + fleet.N <= Nref).all()
    assert same(T.get_initial_state(p), T.get_initial_state(twin)) and same(T.controls(p), T.controls(twin))
