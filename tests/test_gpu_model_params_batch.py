"""One set of model parameters per trajectory (to_set_model_params_batch): every trajectory of a handle is planned on its own
plant.  The reference of every test is B single-trajectory ORACLE problems, problem b built with trajectory b's model and start state
(tests/model_params_fleet.py, the scheme of tests/test_goal_batch.py), with that file's and assert_solve_parity's tolerances: costs rtol
1e-12, gains rtol 1e-7 / atol 1e-9, line-search indices equal, J_new rtol 1e-10; solves: integers equal, cost rtol 1e-8, X / U 1e-6 in
assert_solve_parity's measure (1e-4 for trajectories the oracle itself cut off at an iteration limit).  Rolled-out states and Jacobians
use the bounds of tests/test_gpu_parity.py (1e-11 / 1e-12 and 1e-9 / 1e-11).  Shapes: B = 70 (two tiles, the second with six live
lanes), N = 31 .. 51; parameters within +-20 % of the configuration's, trajectory 0 on the shared values.  The seeds were fixed after
running each fleet on the oracle alone: all of them end SOLVE_SUCCEEDED in every configuration below (the tests ask for >= 90 %).
The flagged instances these configurations do not launch — other integrators, D = 1 and 3, the polish of the other models, the
tangent-matrix layout of the Cartpole, repacked line-search rounds, plants with per-trajectory goals — are in
tests/test_gpu_model_params_instances.py."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import model_params_fleet as F

pytestmark = pytest.mark.gpu
OK = T.capi.SOLVE_SUCCEEDED


def solver_path(p):
    info = np.zeros(8, np.int32)
    p._call("solver_path", p._pi(info))
    return info


def fleet_problem(kind, hip, B, seed, **kw):
    """The batch problem on the shared model with the fleet's models set per trajectory."""
    models = F.draw_models(kind, B, seed)
    p = F.build(kind, hip, B, **kw)
    T.set_model_params(p, models)
    return p, models


# ------------------------------------------------------------------------------------------------ 1. phases
@pytest.mark.parametrize("kind,seed", [("cartpole", 21), ("quadrotor", 22)])
def test_phases_against_per_trajectory_oracle_problems(kind, seed, hip, oracle):
    B, kw = 70, dict(N=41, tf=1.0)
    fl = F.fleet(kind, oracle, B, seed, phases=True, **kw)
    p, models = fleet_problem(kind, hip, B, seed, **kw)
    np.testing.assert_array_equal(T.model_params(p), F.params_of(models))      # to_get_model_params_batch returns what was set
    T.rollout(p)
    np.testing.assert_allclose(T.states(p), fl.Xr, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(T.cost(p), fl.J, rtol=1e-12)
    assert np.ptp(fl.Xr[:, -1, :], axis=0).max() > 1e-3                          # (the plants do differ)
    np.testing.assert_allclose(I.discrete_jacobian(p), fl.F, rtol=1e-9, atol=1e-11)
    # the rolled-out nominal satisfies ITS OWN dynamics at rounding level: 1e-12 is ~100 ulp of the largest state (the defect kernel and the
    # rollout contract their products differently); on the shared model the defect would be the 1e-2 .. 1e-1 the plants differ by
    d = T.dynamics_defect(p)
    assert d.max() < 1e-12, d.max()
    I.expand(p)
    A, Bm = I.dynamics_jacobians(p)
    np.testing.assert_allclose(A, fl.A, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Bm, fl.Bm, rtol=1e-9, atol=1e-11)
    I.backwardpass(p)
    g = I.gains(p)
    np.testing.assert_allclose(g["K"], fl.K, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["d"], fl.d, rtol=1e-7, atol=1e-9)
    ls, Jn = I.forwardpass(p)
    np.testing.assert_array_equal(ls, fl.ls)
    np.testing.assert_allclose(Jn, fl.Jn, rtol=1e-10)


# ------------------------------------------------------------------------------------------------ 2. solves on every layout
#          kind            B    seed  solver   environment                      expected to_solver_path()[0] (0 cooperative, 1 MFMA, 2 lane)
SOLVES = {
    "cartpole_coop": ("cartpole", 70, 11, "ilqr", {}, 0),
    "cartpole_lane": ("cartpole", 300, 12, "ilqr", {"TRAJOPT_BACKWARD": "lane"}, 2),
    "dint_al_bounds": ("dint", 70, 13, "al", {}, 0),
    "cartpole_altro": ("cartpole_con", 70, 14, "altro", {}, 0),
    "quadrotor_mfma": ("quadrotor", 70, 15, "ilqr", {}, 1),
}


def solve_case(case, hip, monkeypatch, guard=None):
    kind, B, seed, solver, env, flavour = SOLVES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if guard is not None:
        monkeypatch.setenv("TRAJOPT_GUARD", guard)
    p, _ = fleet_problem(kind, hip, B, seed)
    info = solver_path(p)
    assert info[0] == flavour and info[1] == 0 and info[5] == 0 and (info[7] & 2) == 0, info
    if case == "quadrotor_mfma":
        assert info[2] == 1, info                                                # active-list compaction stays on the MFMA path
    return F.SOLVERS[solver](p).solve(), p


@pytest.mark.parametrize("case", list(SOLVES))
def test_solves_against_per_trajectory_oracle_problems(case, hip, oracle, monkeypatch):
    kind, B, seed, solver, _, _ = SOLVES[case]
    fl = F.fleet(kind, oracle, B, seed, solver=solver)
    assert (fl.stats["status"] == OK).mean() >= 0.9                              # the oracle alone (vetted before the seed was fixed)
    s, p = solve_case(case, hip, monkeypatch)
    assert (s.stats["status"] == OK).mean() >= 0.9
    F.assert_fleet_parity(s, p, fl, unconverged_rtol=1e-4)
    if solver == "altro":
        np.testing.assert_array_equal(s.stats["iterations_pn"], fl.stats["iterations_pn"])
        assert s.stats["iterations_pn"].max() >= 1 and s.stats["c_max"].max() <= 1e-6   # the polish ran, on each trajectory's own dynamics
    assert np.ptp(T.states(p)[:, -1, :], axis=0).max() > 1e-3 or kind == "cartpole_con"  # (a goal constraint pins the terminal state)


# ------------------------------------------------------------------------------------------------ 3. indexed by trajectory
@pytest.mark.parametrize("kind,seed,env", [("cartpole", 31, {"TRAJOPT_BACKWARD": "lane"}), ("quadrotor", 32, {})])
def test_parameters_matter_and_follow_their_trajectory(kind, seed, env, hip, monkeypatch):
    """Identical start state and goal for every trajectory: what differs between the solved trajectories is the plant alone.  Solving
    with the plants in reversed order returns the reversed results bit for bit — status, iterations, X, U — on the lane layout (separate
    lane kernels) and on the MFMA path with compaction, where finished trajectories leave the active list at different steps."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 70
    models = F.draw_models(kind, B, seed)
    x0 = np.zeros(4) if kind == "cartpole" else np.r_[np.zeros(3), 1.0, np.zeros(9)]
    out = []
    for order in (np.arange(B), np.arange(B)[::-1]):
        p = F.build(kind, hip, B, x0=x0)
        T.set_model_params(p, [models[b] for b in order])
        info = solver_path(p)
        assert info[0] == (2 if kind == "cartpole" else 1) and info[2] == (0 if kind == "cartpole" else 1), info
        s = T.iLQRSolver(p).solve()
        out.append((s.stats["status"].copy(), s.stats["iterations"].copy(), T.states(p), T.controls(p)))
    (st, it, X, U), (str_, itr, Xr, Ur) = out
    assert np.ptp(X[:, -1, :], axis=0).max() > 1e-3                              # well above the 1e-6 parity tolerance
    assert len(np.unique(it)) > 3                                                # ... and they finish at different steps
    np.testing.assert_array_equal(str_[::-1], st)
    np.testing.assert_array_equal(itr[::-1], it)
    np.testing.assert_array_equal(Xr[::-1], X)
    np.testing.assert_array_equal(Ur[::-1], U)


# ------------------------------------------------------------------------------------------------ 4. no history
def _solve_fresh(kind, hip, B, models=None):
    p = F.build(kind, hip, B)
    if models is not None:
        T.set_model_params(p, models)
    s = T.iLQRSolver(p).solve()
    return s.stats["status"].copy(), s.stats["iterations"].copy(), s.stats["cost"].copy(), T.states(p), T.controls(p)


def _resolve(p, kind):
    T.initial_controls(p, T.Quadrotor().hover_control() if kind == "quadrotor" else np.full(1, 0.01))   # the configuration's U0
    s = T.iLQRSolver(p).solve()
    return s.stats["status"].copy(), s.stats["iterations"].copy(), s.stats["cost"].copy(), T.states(p), T.controls(p)


@pytest.mark.parametrize("kind", ["cartpole", "quadrotor"])
def test_set_clear_and_replace_leave_no_history(kind, hip):
    """set -> solve -> clear -> solve equals a fresh shared-parameter handle bit for bit (the rule of tests/test_gpu_handle_reuse.py): the
    scan / fused / packed kernels and the compact cost block are back.  set(A) -> solve -> set(B) -> solve equals a fresh handle with B."""
    B = 70
    A_, B_ = F.draw_models(kind, B, 41), F.draw_models(kind, B, 42)
    p = F.build(kind, hip, B)
    before = solver_path(p).copy()
    T.set_model_params(p, A_)
    T.iLQRSolver(p).solve()
    T.clear_model_params(p)
    np.testing.assert_array_equal(solver_path(p), before)
    np.testing.assert_array_equal(T.model_params(p), np.tile(F.params_of([F.draw_models(kind, 1, 0)[0]]), (B, 1)))
    for got, want in zip(_resolve(p, kind), _solve_fresh(kind, hip, B)):
        np.testing.assert_array_equal(got, want)
    T.set_model_params(p, A_)
    _resolve(p, kind)
    T.set_model_params(p, B_)
    for got, want in zip(_resolve(p, kind), _solve_fresh(kind, hip, B, B_)):
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 5. routing of a large batch
def test_large_batch_created_on_the_lane_layout(hip, oracle):
    """A Cartpole handle created at B = 32 768 sits on the lane layout with the fused kernel, compaction, the two-launch line search and
    the repacked working set; with parameters set it reports none of them, and its solve (flagged k_expand_lane + the separate lane
    backward pass) matches the per-trajectory oracle problems on a seeded sample of 64 trajectories."""
    B, seed, kw = 32768, 51, dict(N=11, tf=0.5)
    p = F.build("cartpole", hip, B, **kw)
    info = solver_path(p)
    assert info[0] == 2 and info[1] == 1 and (info[7] & 2) == 2, info            # as created
    T.set_model_params(p, F.params_of(F.draw_models("cartpole", B, seed)))      # (the [B, 16] array form)
    info = solver_path(p)
    assert info[0] == 2 and info[1] == 0 and info[5] == 0 and (info[7] & 2) == 0, info
    s = T.iLQRSolver(p).solve()
    sel = np.sort(np.random.default_rng(seed).choice(B, 64, replace=False))
    fl = F.fleet("cartpole", oracle, B, seed, solver="ilqr", sel=tuple(int(b) for b in sel), **kw)
    F.assert_fleet_parity(s, p, fl, unconverged_rtol=1e-4, sel=sel)


# ------------------------------------------------------------------------------------------------ 6. guard
@pytest.mark.parametrize("case", ["cartpole_coop", "quadrotor_mfma"])
def test_solves_run_clean_under_the_guard(case, hip, monkeypatch):
    """TRAJOPT_GUARD=1: the per-trajectory array sits between red zones like every other one; the solves run clean and equal the
    unguarded results bit for bit."""
    out = []
    for guard in ("0", "1"):
        s, p = solve_case(case, hip, monkeypatch, guard=guard)
        out.append((s.stats["status"].copy(), s.stats["iterations"].copy(), s.stats["cost"].copy(), T.states(p), T.controls(p)))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. policy rollout default
def test_policy_rollout_simulates_each_trajectory_on_its_own_plant(hip):
    B, S = 70, 3
    p, models = fleet_problem("cartpole", hip, B, 61)
    T.iLQRSolver(p).solve()
    X0s = T.get_initial_state(p)[:, None, :] + np.random.default_rng(61).normal(0.0, 0.02, (B, S, 4))
    own = T.policy_rollout(p, X0s, trajectories=True)
    explicit = T.policy_rollout(p, X0s, trajectories=True, plants=[[models[b]] * S for b in range(B)])
    shared = T.policy_rollout(p, X0s, trajectories=True, plant=T.Cartpole())
    for k in ("J", "c_max", "dx_max", "status", "k_limit", "X", "U"):
        np.testing.assert_array_equal(getattr(own, k), getattr(explicit, k), err_msg=k)
    # trajectory 0 IS on the shared model (another kernel instance — per-lane plant against broadcast plant — so equal to rounding, not bit
    # for bit); the others are not
    np.testing.assert_allclose(own.X[0], shared.X[0], rtol=1e-9, atol=1e-11)
    assert np.abs(own.X[1:] - shared.X[1:]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(hip):
    from test_hybrid_dims import hybrid_problem
    from test_infeasible import cartpole_infeasible
    from test_model_vector import build as vector_problem, cartpole_mix

    def rigid(rotation):
        model = T.Quadrotor(rotation=rotation)
        n, m = model.dims()
        obj = T.LQRObjective(np.ones(n), np.ones(m), np.ones(n), np.zeros(n), 11)
        return T.Problem(model, obj, model.build_state([0.0, 0.0, 1.0]), 1.0, batch=3, lib=hip)
    refused = [(rigid("mrp"), "Quadrotor.MRP."), (rigid("rp"), "Quadrotor.RodriguesParam."), (hybrid_problem(hip)[0], "hybrid double integrator"),
               (vector_problem(cartpole_mix(), hip)[0], "model vector"), (cartpole_infeasible(hip)[0], "InfeasibleModel .Cartpole.")]
    for p, name in refused:
        for call in (lambda: T.set_model_params(p, np.zeros((p.B, 16))), lambda: T.model_params(p), lambda: T.clear_model_params(p)):
            with pytest.raises(T.UnsupportedError, match=name):
                call()
    # entries that select dimensions or the attitude representation must be the problem's; the first offending trajectory is named
    p = F.build("dint", hip, 5)
    pp = T.model_params(p)
    bad = pp.copy(); bad[3, 1] = 3.0
    with pytest.raises(T.ArgumentError, match="trajectory 3 change the model's dimensions"):
        p._call("set_model_params_batch", p._pd(bad))
    q = F.build("quadrotor", hip, 5)
    qq = T.model_params(q)
    bad = qq.copy(); bad[2, 10] = 1.0; bad[4, 10] = 2.0
    with pytest.raises(T.ArgumentError, match="trajectory 2 change the model's dimensions or attitude"):
        q._call("set_model_params_batch", q._pd(bad))
    bad = qq.copy(); bad[4, 0] = np.nan
    with pytest.raises(T.ArgumentError, match="entry 0 of trajectory 4 is not finite"):
        q._call("set_model_params_batch", q._pd(bad))                           # (past the wrapper's own check: the library's)
    with pytest.raises(ValueError, match="null pointer"):
        q._call("set_model_params_batch", None)
    np.testing.assert_array_equal(T.model_params(q), qq)                         # nothing was set by the refused calls
    assert (solver_path(q)[7] & 1) == 1 and solver_path(q)[1] == 0
    # a solve in flight: like every other handle call
    big = F.build("quadrotor", hip, 256, N=101, tf=5.0)
    models = F.draw_models("quadrotor", 256, 71)
    s = T.iLQRSolver(big).solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="in flight"):
            T.set_model_params(big, models)
    finally:
        s.wait()
    T.set_model_params(big, models)                                             # ... and fine once it has ended
