"""to_mpc_advance on the MI355X: the receding-horizon step on the device against the host recipe it replaces.

The reference is always a TWIN handle driven through entry points that exist without the feature and that it leaves unchanged: the same
solve, ``T.policy_rollout(twin, x_meas[:, None, :], trajectories=True, ...)``, the shift written out in numpy below (``shifted``),
``set_initial_state``, ``initial_controls`` and ``T.rollout``.  The advance launches the same policy-kernel instances and then only copies
what they computed, so every comparison is equality of BITS (``same``: floats are compared as 64-bit patterns) — no measured number enters
a tolerance.  The one exception is stated where it is made: closed-loop and nominal guess agree to 1e-12 when the closed loop applies the
nominal controls, the tolerance of tests/test_gpu_policy_rollout.py::test_nominal_sample_is_the_open_loop_rollout for the same statement."""
import ctypes as C

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import capi
from trajectoryoptimization_jl_amd import configs

pytestmark = pytest.mark.gpu

INT_STATS = ("iterations", "iterations_outer", "status", "iterations_pn")


# ------------------------------------------------------------------------------------------------ problems
def double_integrator_problem(lib, batch, N=11, options=None):
    model = T.DoubleIntegrator(1.0, 2)
    n, m = model.dims()
    xf = np.array([1.0, 2.0, 0.0, 0.0])
    obj = T.LQRObjective(np.ones(n), np.full(m, 0.1), np.full(n, 10.0), xf, N)
    p = T.Problem(model, obj, np.zeros(n), 2.0, xf=xf, batch=batch, lib=lib, options=options)
    rng = np.random.default_rng(3)
    p.set_initial_state(rng.uniform(-0.5, 0.5, (batch, n)))
    T.initial_controls(p, np.zeros(m))
    return p


MODELS = {
    "double_integrator": (lambda lib, B, **kw: double_integrator_problem(lib, B, N=11, **kw), T.iLQRSolver, dict(iterations=10)),
    "cartpole": (lambda lib, B, **kw: configs.cartpole_problem(batch=B, N=21, tf=2.0, lib=lib, **kw), T.iLQRSolver, dict(iterations=15)),
    "quadrotor": (lambda lib, B, **kw: configs.quadrotor_problem(batch=B, N=15, tf=1.0, lib=lib, **kw), T.iLQRSolver, dict(iterations=8)),
    "cartpole_al": (lambda lib, B, **kw: configs.cartpole_problem(batch=B, N=21, tf=2.0, constrained=True, lib=lib, **kw), T.ALSolver, dict()),
}


def same(a, b):
    """Equality of bits (a NaN equals the same NaN, -0.0 does not equal 0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return bool(np.array_equal(a, b))


def handle_state(p):
    return dict(x0=T.get_initial_state(p), U=T.controls(p), X=T.states(p))


def assert_same_handles(p, twin, what=""):
    a, b = handle_state(p), handle_state(twin)
    for k in a:
        assert same(a[k], b[k]), f"{what}: {k} of the two handles differs in {int((a[k] != b[k]).sum())} entries"


def solved_pair(case, B, hip, prepare=None, count=2, **build_kw):
    """`count` handles of the same problem after the same solve (asserted: the twin is a twin)."""
    build, solver, skw = MODELS[case]
    out = []
    for _ in range(count):
        p = build(hip, B, **build_kw)
        if prepare is not None:
            prepare(p)
        s = solver(p, **skw)
        s.solve()
        out.append((p, s))
    for p, s in out[1:]:
        for k in INT_STATS:
            assert np.array_equal(s.stats[k], out[0][1].stats[k]), k
        assert_same_handles(out[0][0], p, "after the first solve")
    return out


def measured(p, scale=0.02, seed=17):
    """A measured state next to the handle's x0 (unit quaternion kept)."""
    x = T.get_initial_state(p) + scale * np.random.default_rng(seed).standard_normal((p.B, p.n))
    if isinstance(p.model, T.Quadrotor) and p.n == 13:
        x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=-1, keepdims=True)
    return np.ascontiguousarray(x)


def shifted(V, s, tail, u_fill):
    """The warm-start shift, written out: Unew[k] = V[k + s] while k + s <= N-2, else the tail.  V [B, N-1, m]."""
    K = V.shape[1]
    out = np.empty_like(V)
    for k in range(K):
        if k + s <= K - 1:
            out[:, k] = V[:, k + s]
        elif tail == "hold":
            out[:, k] = V[:, K - 1]
        else:
            out[:, k] = u_fill
    return out


def host_recipe(twin, x_meas, s=1, guess="closed_loop", tail="hold", u_fill=None, **policy_kw):
    """INTEGRATION.md's MPC step on the host, through T.policy_rollout and the setters.  Returns the rollout."""
    x0_old, U_old = T.get_initial_state(twin), T.controls(twin)
    xm = x0_old if x_meas is None else x_meas
    r = T.policy_rollout(twin, np.ascontiguousarray(xm[:, None, :]), trajectories=True, **policy_kw)
    ok = r.status[:, 0] == 0
    U_new = shifted(r.U[:, 0] if guess == "closed_loop" else U_old, s, tail, None if u_fill is None else np.broadcast_to(np.asarray(u_fill, float), (twin.m,)))
    twin.set_initial_state(np.where(ok[:, None], r.X[:, 0, s], x0_old))
    T.initial_controls(twin, np.where(ok[:, None, None], U_new, U_old))
    T.rollout(twin)
    return r


def assert_advance_equals_recipe(a, r, s, what=""):
    """MpcAdvance against the corresponding slices of the twin's rollout."""
    for k, want in (("x_next", r.X[:, 0, s]), ("X", r.X[:, 0, :s + 1]), ("U", r.U[:, 0, :s]), ("J", r.J[:, 0]), ("c_max", r.c_max[:, 0]),
                    ("dx_max", r.dx_max[:, 0]), ("status", r.status[:, 0]), ("k_limit", r.k_limit[:, 0])):
        assert same(getattr(a, k), want), f"{what}: {k}"


def advance_both(p, twin, x_meas, what="", **kw):
    a = T.mpc_advance(p, x_meas, **{("shift" if k == "s" else k): v for k, v in kw.items()})
    r = host_recipe(twin, x_meas, **kw)
    assert_advance_equals_recipe(a, r, kw.get("s", 1), what)
    assert_same_handles(p, twin, what)
    return a, r


def assert_following_solves_agree(sp, stwin, what=""):
    sp.solve(); stwin.solve()
    for k in INT_STATS:
        assert np.array_equal(sp.stats[k], stwin.stats[k]), f"{what}: {k} of the following solve"
    assert (sp.total_iterations, sp.batch_steps) == (stwin.total_iterations, stwin.batch_steps), what
    assert same(sp.stats["cost"], stwin.stats["cost"]) and same(sp.stats["c_max"], stwin.stats["c_max"]), what
    assert_same_handles(sp.prob, stwin.prob, what + " after the following solve")


# ------------------------------------------------------------------------------------------------ 1. models and batches
@pytest.mark.parametrize("B", [1, 65, 130])
@pytest.mark.parametrize("case", ["double_integrator", "cartpole", "quadrotor"])
def test_advance_equals_the_host_recipe(case, B, hip):
    (p, sp), (twin, stwin) = solved_pair(case, B, hip)
    a, _ = advance_both(p, twin, measured(p), what=f"{case} B={B}")
    assert np.all(a.status == 0)
    assert same(p.x0, T.get_initial_state(p))                      # the host's copy of x0 follows the handle
    assert_following_solves_agree(sp, stwin, f"{case} B={B}")


# ------------------------------------------------------------------------------------------------ 2. chunks
def test_chunks_of_one_wave_equal_one_chunk(hip, monkeypatch):
    (p1, _), (p3, _), (twin, _) = solved_pair("cartpole", 130, hip, count=3)
    xm = measured(p1)
    a1 = T.mpc_advance(p1, xm, shift=2)                            # no override: all three waves in one chunk
    monkeypatch.setenv("TRAJOPT_POLICY_CHUNK_WAVES", "1")          # three chunks; the staging pair is re-used in stream order
    a3 = T.mpc_advance(p3, xm, shift=2)
    monkeypatch.delenv("TRAJOPT_POLICY_CHUNK_WAVES")
    r = host_recipe(twin, xm, s=2)
    assert_advance_equals_recipe(a1, r, 2, "one chunk")
    assert_advance_equals_recipe(a3, r, 2, "three chunks")
    assert_same_handles(p1, twin, "one chunk")
    assert_same_handles(p3, twin, "three chunks")


# ------------------------------------------------------------------------------------------------ 3. shifts, tails, guesses
@pytest.mark.parametrize("guess", ["closed_loop", "nominal"])
@pytest.mark.parametrize("tail", ["hold", "fill"])
@pytest.mark.parametrize("s", [1, 3, 19])                          # N = 21: 19 = N - 2
def test_shifts_tails_and_guesses(s, tail, guess, hip):
    (p, sp), (twin, stwin) = solved_pair("cartpole", 65, hip)
    advance_both(p, twin, measured(p), what=f"s={s} {tail} {guess}", s=s, tail=tail, guess=guess, u_fill=0.125 if tail == "fill" else None)
    assert_following_solves_agree(sp, stwin, f"s={s} {tail} {guess}")


def test_fill_takes_a_vector_per_control(hip):
    (p, _), (twin, _) = solved_pair("quadrotor", 65, hip)
    fill = np.array([1.0, -0.0, 2.5, 1e-300])
    advance_both(p, twin, measured(p), what="quadrotor fill", s=3, tail="fill", guess="nominal", u_fill=fill)
    assert same(T.controls(p)[:, -3:], np.broadcast_to(fill, (65, 3, 4)))


# ------------------------------------------------------------------------------------------------ 4. x_meas = None
def test_no_measurement_starts_from_the_handles_x0(hip):
    (p, _), (q, _), (pn, _) = solved_pair("cartpole", 65, hip, count=3)
    a = T.mpc_advance(p, shift=2)
    b = T.mpc_advance(q, T.get_initial_state(q), shift=2)
    for k in ("x_next", "X", "U", "J", "c_max", "dx_max", "status", "k_limit"):
        assert same(getattr(a, k), getattr(b, k)), k
    assert_same_handles(p, q, "x_meas = None against T.get_initial_state")
    # planning plant, alpha = 0, no noise, from x0: dx stays 0 and the closed loop applies the nominal controls, so the closed-loop guess
    # is the nominal guess to rounding (1e-12: test_nominal_sample_is_the_open_loop_rollout's tolerance for the same statement)
    T.mpc_advance(pn, shift=2, guess="nominal")
    np.testing.assert_allclose(T.controls(p), T.controls(pn), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(T.get_initial_state(p), T.get_initial_state(pn), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(T.states(p), T.states(pn), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 5. clamp, plant, noise
def test_clamp_and_a_mismatched_plant(hip):
    (p, sp), (twin, stwin) = solved_pair("cartpole", 65, hip)
    kw = dict(u_min=-0.5, u_max=0.75, plant=T.Cartpole(mc=1.1, mp=0.3, l=0.45), alpha=0.5)
    a, r = advance_both(p, twin, measured(p), what="clamp + plant", s=3, **kw)
    assert r.U.min() == -0.5 and r.U.max() == 0.75, "the clamp never acted: the case checks nothing"
    assert_following_solves_agree(sp, stwin, "clamp + plant")


def test_noise_with_a_sample_offset(hip):
    (p, sp), (twin, stwin) = solved_pair("cartpole", 65, hip)
    noise = lambda: T.PolicyNoise(11, sigma_w=0.01, sigma_v=[0.02, 0.01, 0.0, 0.03], sample_offset=3)
    (q, _), = solved_pair("cartpole", 65, hip, count=1)
    xm = measured(p)
    a, _ = advance_both(p, twin, xm, what="noise", s=2, noise=noise())
    quiet = T.mpc_advance(q, xm, shift=2)
    assert not same(a.x_next, quiet.x_next), "the noise did not act"
    assert_following_solves_agree(sp, stwin, "noise")


# ------------------------------------------------------------------------------------------------ 6. per-trajectory arrays
def test_per_trajectory_plants_time_steps_and_goals(hip):
    B = 65
    def prepare(p):
        T.set_model_params(p, [T.Cartpole(mp=0.2 + 0.002 * b, l=0.5 - 0.001 * b) for b in range(B)])
        T.set_time_steps_batch(p, 0.1 * (1.0 + 0.3 * np.sin(np.arange(B)[:, None] + 0.5 * np.arange(p.N - 1)[None, :])))
        xf = np.tile(np.array([0.0, np.pi, 0.0, 0.0]), (B, 1))
        xf[:, 0] = np.linspace(-0.5, 0.5, B)
        T.set_goal_state(p, xf)                                   # per-trajectory q: J of the rollout reads gl
    (p, sp), (twin, stwin) = solved_pair("cartpole", B, hip, prepare=prepare)
    keep = (T.model_params(p), T.time_steps(p))
    a, r = advance_both(p, twin, measured(p), what="per-trajectory arrays", s=2)
    assert np.all(a.status == 0) and len(np.unique(a.J)) > B // 2
    assert same(T.model_params(p), keep[0]) and same(T.time_steps(p), keep[1])   # the plan moves, the grid and the plants do not
    assert_following_solves_agree(sp, stwin, "per-trajectory arrays")


# ------------------------------------------------------------------------------------------------ 7. AL solves
def test_between_two_al_solves(hip):
    from trajopt_amd import internal as I
    (p, sp), (twin, stwin) = solved_pair("cartpole_al", 65, hip)
    assert same(sp.stats["c_max"], stwin.stats["c_max"])
    duals = [I.get_duals(p, i) for i in range(len(p.constraints))]
    a, r = advance_both(p, twin, measured(p), what="AL", s=2)
    assert np.all(np.isfinite(a.c_max))
    for i, (lam, mu) in enumerate(duals):                          # duals and penalties are not shifted
        lam2, mu2 = I.get_duals(p, i)
        assert same(lam, lam2) and same(mu, mu2), f"constraint {i}"
    assert_following_solves_agree(sp, stwin, "AL")


# ------------------------------------------------------------------------------------------------ 8. limit events
def test_a_trajectory_beyond_the_limit_stays_where_it_is(hip):
    B, limit = 65, 1e2
    kw = dict(options=T.SolverOptions(lib=hip, max_state_value=limit))
    build = lambda lib, b, **k: configs.cartpole_problem(batch=b, N=21, tf=2.0, lib=lib, **k)
    pairs = []
    for _ in range(2):
        p = build(hip, B, **kw)
        s = T.iLQRSolver(p, iterations=15)
        s.solve()
        pairs.append((p, s))
    (p, sp), (twin, stwin) = pairs
    assert_same_handles(p, twin, "after the first solve")
    xm = measured(p)
    xm[[0, 64], 0] = 10 * limit                                    # the first step arrives beyond the limit whatever the law does
    before = handle_state(p)
    a = T.mpc_advance(p, xm, shift=2)
    r = host_recipe(twin, xm, s=2)
    bad = r.status[:, 0] != 0
    assert np.array_equal(np.flatnonzero(bad), [0, 64]), "the condition of this test: exactly these two leave the limits in the twin"
    assert_advance_equals_recipe(a, r, 2, "limit")
    assert np.all(a.status[bad] == capi.STATE_LIMIT) and np.all(a.k_limit[bad] == 1) and np.all(np.isposinf(a.J[bad]))
    after = handle_state(p)
    for k in ("x0", "U"):
        assert same(after[k][bad], before[k][bad]), f"{k} of a trajectory beyond the limit changed"
        assert not np.any([same(after[k][b], before[k][b]) for b in np.flatnonzero(~bad)]), f"{k}: one of the other 63 did not advance"
    assert same(p.x0, after["x0"])
    assert_same_handles(p, twin, "limit")


# ------------------------------------------------------------------------------------------------ 9. the closed loop
def test_mpc_run_equals_the_host_composed_loop(hip):
    B, steps, s, seed = 8, 4, 2, 2024
    plant = T.Cartpole(mc=1.2, mp=0.24)                            # 20 % heavier than the planning model
    hooks = []
    p = configs.cartpole_problem(batch=B, N=21, tf=2.0, lib=hip)
    twin = configs.cartpole_problem(batch=B, N=21, tf=2.0, lib=hip)
    sp, stwin = T.iLQRSolver(p, iterations=15), T.iLQRSolver(twin, iterations=15)
    rec = T.mpc_run(sp, steps, shift=s, plant=plant, noise=T.PolicyNoise(seed, sigma_w=0.005), before_solve=lambda prob, t: hooks.append((prob is p, t)))
    assert hooks == [(True, t) for t in range(steps)]
    X_cl, U_cl = np.empty((B, steps * s + 1, p.n)), np.empty((B, steps * s, p.m))
    its, sts = np.empty((steps, B), np.int32), np.empty((steps, B), np.int32)
    for t in range(steps):
        stwin.solve()
        its[t], sts[t] = stwin.stats["iterations"], stwin.stats["status"]
        r = host_recipe(twin, None, s=s, plant=plant, noise=T.PolicyNoise(seed, sigma_w=0.005, sample_offset=t))
        assert np.all(r.status == 0)
        if t == 0:
            X_cl[:, 0] = r.X[:, 0, 0]
        X_cl[:, t * s + 1:(t + 1) * s + 1], U_cl[:, t * s:(t + 1) * s] = r.X[:, 0, 1:s + 1], r.U[:, 0, :s]
    assert same(rec.X_cl, X_cl) and same(rec.U_cl, U_cl)
    assert np.array_equal(rec.iterations, its) and np.array_equal(rec.status, sts) and not np.any(rec.advance_status)
    assert_same_handles(p, twin, "after four periods")
    # the record is continuous: every period starts where the last one arrived
    assert same(rec.X_cl[:, -1], T.get_initial_state(p))


# ------------------------------------------------------------------------------------------------ 10. guard
def test_runs_clean_under_the_guard(hip, monkeypatch):
    out = []
    for guard in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_GUARD", guard)
        monkeypatch.setenv("TRAJOPT_POLICY_CHUNK_WAVES", "1")      # the staging pair at its smallest: a row too far leaves it
        p = configs.cartpole_problem(batch=130, N=21, tf=2.0, lib=hip)
        s = T.iLQRSolver(p, iterations=15)
        s.solve()
        xm = measured(p)
        a = T.mpc_advance(p, xm, shift=3, tail="fill", u_fill=0.0)
        b = T.mpc_advance(p, shift=19, guess="nominal")            # the longest shift on the same handle (staging re-used, larger gather)
        s.solve()
        out.append((a, b, handle_state(p), {k: v.copy() for k, v in s.stats.items()}))
    for k in ("x_next", "X", "U", "J", "status"):
        assert same(getattr(out[0][0], k), getattr(out[1][0], k)) and same(getattr(out[0][1], k), getattr(out[1][1], k)), k
    for k in out[0][2]:
        assert same(out[0][2][k], out[1][2][k]), k
    for k in INT_STATS:
        assert np.array_equal(out[0][3][k], out[1][3][k]), k


# ------------------------------------------------------------------------------------------------ 11. refusals
def _raw(p, x_meas=None, mpc=None, popts=None, noise=None, out=None):
    ref = lambda o: None if o is None else C.byref(o)
    p._call("mpc_advance", None if x_meas is None else p._pd(x_meas), ref(mpc), ref(popts), ref(noise), ref(out))


def _mpc(shift=1, guess=0, tail=0, reserved=0, u_fill=None):
    o = capi.MpcOpts()
    o.shift, o.guess, o.tail, o.reserved = shift, guess, tail, reserved
    if u_fill is not None:
        o._keep = np.ascontiguousarray(u_fill, dtype=np.float64)
        o.u_fill = o._keep.ctypes.data_as(C.POINTER(C.c_double))
    return o


def test_refusals(hip):
    p = configs.cartpole_problem(batch=5, N=11, tf=1.0, lib=hip)
    T.iLQRSolver(p, iterations=3).solve()
    before = handle_state(p)
    rows = [
        (dict(mpc=_mpc(shift=0)), T.ArgumentError, r"to_mpc_advance: shift must be in 1 \.\. N-2 = 9"),
        (dict(mpc=_mpc(shift=10)), T.ArgumentError, "to_mpc_advance: shift"),
        (dict(mpc=_mpc(shift=-1)), T.ArgumentError, "to_mpc_advance: shift"),
        (dict(mpc=_mpc(guess=2)), T.ArgumentError, "to_mpc_advance: guess"),
        (dict(mpc=_mpc(guess=-1)), T.ArgumentError, "to_mpc_advance: guess"),
        (dict(mpc=_mpc(tail=2)), T.ArgumentError, "to_mpc_advance: tail"),
        (dict(mpc=_mpc(reserved=1)), T.ArgumentError, "to_mpc_advance: reserved must be 0"),
        (dict(mpc=None), ValueError, "to_mpc_advance: mpc is NULL"),
        (dict(mpc=_mpc(tail=1)), ValueError, "to_mpc_advance: TO_MPC_TAIL_FILL needs u_fill"),
        (dict(mpc=_mpc(tail=1, u_fill=[np.nan])), T.ArgumentError, "to_mpc_advance: u_fill must be finite"),
        (dict(mpc=_mpc(tail=1, u_fill=[np.inf])), T.ArgumentError, "to_mpc_advance: u_fill must be finite"),
    ]
    for kw, err, match in rows:
        with pytest.raises(err, match=match) as e:
            _raw(p, **kw)
        assert type(e.value) is err, (match, type(e.value))      # (TO_ERR_NULL is a plain ValueError, TO_ERR_ARGUMENT its subclass)
    # what to_policy_rollout_mc refuses, with its error
    po = capi.PolicyOpts()
    po.refresh_gains, po.alpha = 2, 0.0
    with pytest.raises(T.ArgumentError, match="refresh_gains must be 0 or 1"):
        _raw(p, mpc=_mpc(), popts=po)
    po.refresh_gains, po.alpha = 1, float("inf")
    with pytest.raises(T.ArgumentError, match="alpha must be finite"):
        _raw(p, mpc=_mpc(), popts=po)
    with pytest.raises(T.ArgumentError, match="u_min must not exceed u_max"):
        T.mpc_advance(p, u_min=1.0, u_max=-1.0)
    with pytest.raises(T.ArgumentError, match="sigma_w must be finite and >= 0"):
        T.mpc_advance(p, noise=T.PolicyNoise(1, sigma_w=-0.1))
    q = double_integrator_problem(hip, 3)
    with pytest.raises(T.ArgumentError, match="change the model's dimensions"):
        _raw(q, mpc=_mpc(), popts=_plant_opts(np.r_[1.0, 3.0, np.zeros(14)]))    # a plant of another D
    after = handle_state(p)
    for k in before:
        assert same(before[k], after[k]), f"a refused call changed {k}"
    # out == NULL and popts == NULL are no refusals
    _raw(p, mpc=_mpc())
    assert not same(T.get_initial_state(p), before["x0"])


def _plant_opts(pp):
    o = capi.PolicyOpts()
    o.refresh_gains = 1
    o._keep = np.ascontiguousarray(pp, dtype=np.float64)
    o.plant_params = o._keep.ctypes.data_as(C.POINTER(C.c_double))
    return o


def test_models_that_cannot_shift_are_refused_by_name(hip):
    from test_hybrid_dims import hybrid_problem
    from test_model_vector import build as vector_problem, cartpole_mix
    hyb = hybrid_problem(hip, batch=3)[0]
    vec = vector_problem(cartpole_mix(), hip, batch=3)[0]
    base = configs.cartpole_problem(batch=3, N=11, tf=1.0, constrained=True, lib=hip)
    T.rollout(base)
    inf = T.InfeasibleProblem(base, T.states(base), R_inf=1.0)
    for prob, name in ((hyb, "hybrid double integrator"), (vec, "model vector"), (inf, r"InfeasibleModel \(Cartpole\)")):
        T.rollout(prob)
        before = handle_state(prob)
        with pytest.raises(T.UnsupportedError, match="to_mpc_advance: not available for the " + name):
            T.mpc_advance(prob)
        after = handle_state(prob)
        assert all(same(before[k], after[k]) for k in before)


def test_a_solve_in_flight_refuses(hip):
    p = configs.cartpole_problem(batch=65, N=21, tf=2.0, lib=hip)
    s = T.iLQRSolver(p, iterations=15)
    s.solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="to_mpc_advance: an asynchronous solve is in flight"):
            T.mpc_advance(p)
    finally:
        s.wait()
    assert np.all(T.mpc_advance(p).status == 0)


# ------------------------------------------------------------------------------------------------ 12. isolation
def test_a_handle_that_advanced_solves_like_one_that_was_set(hip):
    """A handle that never calls to_mpc_advance and one that did — and then had x0 and U set to the same values through the setters —
    solve bit-identically: the advance leaves nothing behind but x0, U and their rollout."""
    (p, sp), (fresh, sfresh) = solved_pair("cartpole", 65, hip)
    T.mpc_advance(p, measured(p), shift=3, tail="fill", u_fill=0.0, noise=T.PolicyNoise(5, sigma_w=0.01))
    x0, U = T.get_initial_state(p), T.controls(p)
    for q in (p, fresh):
        q.set_initial_state(x0)
        T.initial_controls(q, U)
        T.rollout(q)
    assert_same_handles(p, fresh, "after the setters")
    assert_following_solves_agree(sp, sfresh, "isolation")
