"""One set of time steps per trajectory (to_set_time_steps_batch): every trajectory of a handle is planned on its own
horizon.  The reference of every test is B single-trajectory ORACLE problems, problem b built with ``dt = dt_b`` and trajectory b's start
state (tests/time_step_fleets.py, the scheme of tests/model_params_fleet.py), with that file's and assert_fleet_parity's tolerances: costs
rtol 1e-12, gains rtol 1e-7 / atol 1e-9, line-search indices equal, J_new rtol 1e-10, rolled-out states 1e-11 / 1e-12, Jacobians 1e-9 /
1e-11; solves: integers equal, cost rtol 1e-8, X / U 1e-6 in assert_solve_parity's measure (1e-4 for trajectories the oracle itself cut off
at an iteration limit).  Shapes: B = 70 (two tiles, the second with six live lanes), B = 300 on the lane layout, N = 31 .. 51.  Step
fleets: uniform (tf_b within +-25 % of the configuration's) and ragged (another grid per trajectory AND per knot).  The seeds were fixed
after running each fleet on the oracle alone (tests/test_time_steps_oracle.py): all of them end SOLVE_SUCCEEDED in every configuration (the
tests ask for >= 90 %).  Several configurations scale their stage costs by dt (cost_dt_scaling), so that the cost kernels' reads of the
step are compared as well."""
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import model_params_fleet as M
import time_step_fleets as F

pytestmark = pytest.mark.gpu
OK = T.capi.SOLVE_SUCCEEDED
GOLDEN = Path(__file__).resolve().parent / "golden" / "pm_only_parent.npz"


def solver_path(p):
    info = np.zeros(8, np.int32)
    p._call("solver_path", p._pi(info))
    return info


def results(s, p):
    return s.stats["status"].copy(), s.stats["iterations"].copy(), s.stats["cost"].copy(), T.states(p), T.controls(p)


def assert_same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------------ 1. phases
@pytest.mark.parametrize("kind", list(F.PHASES))
def test_phases_against_per_trajectory_oracle_problems(kind, hip, oracle):
    B = 70
    fl = F.phase_fleet(kind, oracle)
    p = M.build(kind, hip, B, **F.PHASE_KW[kind])
    shared = T.time_steps(p)
    np.testing.assert_array_equal(shared, np.full((B, 40), 1.0 / 40))              # the descriptor's steps, repeated
    T.set_time_steps_batch(p, fl.dt)
    np.testing.assert_array_equal(T.time_steps(p), fl.dt)                          # to_get_time_steps_batch returns what was set
    T.rollout(p)
    np.testing.assert_allclose(T.states(p), fl.Xr, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(T.cost(p), fl.J, rtol=1e-12)
    np.testing.assert_allclose(T.stage_costs(p), fl.Jk, rtol=1e-12, atol=1e-300)
    assert np.ptp(fl.Xr[:, -1, :], axis=0).max() > 1e-2                            # (the horizons do differ)
    np.testing.assert_allclose(I.discrete_jacobian(p), fl.F, rtol=1e-9, atol=1e-11)
    # the rolled-out nominal satisfies ITS OWN dynamics at rounding level; on the shared steps the defect would be ~1e-2
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
def solve_case(case, ragged, hip, monkeypatch, guard=None):
    kind, B, seed, solver, env, flavour, options = F.SOLVES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if guard is not None:
        monkeypatch.setenv("TRAJOPT_GUARD", guard)
    p = M.build(kind, hip, B, **F.okw(options))
    dt, tf = F.steps_of(kind, B, seed, ragged)
    if ragged:
        T.set_time_steps_batch(p, dt)
    else:
        T.set_final_times_batch(p, tf)
        np.testing.assert_array_equal(T.time_steps(p), dt)
    info = solver_path(p)
    assert info[0] == flavour and info[1] == 0 and info[5] == 0 and (info[7] & 2) == 0, info     # no fused, no scan, no repacked set
    if case == "quadrotor_mfma":
        assert info[2] == 1, info                                                # active-list compaction stays on the MFMA path
    return M.SOLVERS[solver](p).solve(), p


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "uniform"])
@pytest.mark.parametrize("case", list(F.SOLVES))
def test_solves_against_per_trajectory_oracle_problems(case, ragged, hip, oracle, monkeypatch):
    kind, solver = F.SOLVES[case][0], F.SOLVES[case][3]
    fl = F.solve_fleet(case, oracle, ragged)
    assert (fl.stats["status"] == OK).mean() >= 0.9                              # the oracle alone (vetted before the seed was fixed)
    s, p = solve_case(case, ragged, hip, monkeypatch)
    assert (s.stats["status"] == OK).mean() >= 0.9
    M.assert_fleet_parity(s, p, fl, unconverged_rtol=1e-4)
    if solver == "altro":
        np.testing.assert_array_equal(s.stats["iterations_pn"], fl.stats["iterations_pn"])
        assert s.stats["iterations_pn"].max() >= 1 and s.stats["c_max"].max() <= 1e-6   # the polish ran, on each trajectory's own steps
    assert np.ptp(T.states(p)[:, -1, :], axis=0).max() > 1e-3 or kind == "cartpole_con"  # (a goal constraint pins the terminal state)


# ------------------------------------------------------------------------------------------------ 3. indexed by trajectory
@pytest.mark.parametrize("kind,env", [("cartpole", {"TRAJOPT_BACKWARD": "lane"}), ("quadrotor", {})])
def test_steps_matter_and_follow_their_trajectory(kind, env, hip, monkeypatch):
    """Identical start state, goal and plant for every trajectory: what differs between the solved trajectories is the time steps alone.
    Solving with the steps in reversed order returns the reversed results bit for bit — status, iterations, X, U — on the lane layout
    (separate lane kernels) and on the MFMA path with compaction, where finished trajectories leave the active list at different steps."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B = 70
    dt, _ = F.steps_of(kind, B, F.ORDER[kind], True)
    x0 = np.zeros(4) if kind == "cartpole" else np.r_[np.zeros(3), 1.0, np.zeros(9)]
    out = []
    for order in (np.arange(B), np.arange(B)[::-1]):
        p = M.build(kind, hip, B, x0=x0)
        T.set_time_steps_batch(p, dt[order])
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


# ------------------------------------------------------------------------------------------------ 4. same instances, same bits
def _solve(p, solver="ilqr"):
    return results(M.SOLVERS[solver](p).solve(), p)


@pytest.mark.parametrize("kind,solver", [("cartpole", "ilqr"), ("quadrotor", "ilqr"), ("cartpole_con", "altro")])
def test_descriptor_steps_equal_a_plants_handle_on_the_shared_model(kind, solver, hip):
    """Steps set to the descriptor's own values run the instances a handle with to_set_model_params_batch of the shared model runs, on the
    same numbers: bit-identical results."""
    B = 70
    a = M.build(kind, hip, B)
    T.set_model_params(a, M.draw_models(kind, B, 0, spread=0.0))
    b = M.build(kind, hip, B)
    T.set_time_steps_batch(b, T.time_steps(b))
    np.testing.assert_array_equal(solver_path(a), solver_path(b))
    np.testing.assert_array_equal(T.model_params(b), T.model_params(a))          # (the shared plant, repeated)
    assert_same(_solve(a, solver), _solve(b, solver))


@pytest.mark.parametrize("kind", ["cartpole", "quadrotor"])
def test_clear_leaves_no_history(kind, hip):
    """set -> solve -> clear -> solve equals a fresh handle bit for bit: the scan / fused / packed kernels are back.  With plants set as
    well, clearing the steps leaves the plants (and the other way round)."""
    B = 70
    dt, _ = F.steps_of(kind, B, 161, True)
    U0 = T.Quadrotor().hover_control() if kind == "quadrotor" else np.full(1, 0.01)
    p = M.build(kind, hip, B)
    before = solver_path(p).copy()
    T.set_time_steps_batch(p, dt)
    T.iLQRSolver(p).solve()
    T.clear_time_steps_batch(p)
    np.testing.assert_array_equal(solver_path(p), before)
    np.testing.assert_array_equal(T.time_steps(p), T.time_steps(M.build(kind, hip, B)))
    T.initial_controls(p, U0)
    assert_same(_solve(p), _solve(M.build(kind, hip, B)))
    # plants + steps, then one of the two cleared: what stays is what a fresh handle with it alone computes
    models = M.draw_models(kind, B, 162)
    for clear, keep in ((T.clear_time_steps_batch, lambda q: T.set_model_params(q, models)), (T.clear_model_params, lambda q: T.set_time_steps_batch(q, dt))):
        p = M.build(kind, hip, B)
        T.set_model_params(p, models); T.set_time_steps_batch(p, dt)
        clear(p)
        q = M.build(kind, hip, B)
        keep(q)
        np.testing.assert_array_equal(T.model_params(p), T.model_params(q))
        np.testing.assert_array_equal(T.time_steps(p), T.time_steps(q))
        assert_same(_solve(p), _solve(q))


def test_plants_only_handle_computes_what_it_did_before_time_steps_existed(hip):
    """tests/golden/pm_only_parent.npz holds the results of handles with to_set_model_params_batch alone — Cartpole iLQR (B = 70, seed 11),
    constrained Cartpole ALTRO (B = 70, seed 14) and Quadrotor iLQR (B = 70, seed 15; the first 16 trajectories' X / U), the fleets of
    tests/test_gpu_model_params_batch.py — recorded with tools/pm_only_golden.py on an MI355X from the library built at the commit before
    per-trajectory time steps were added.  The flagged instances now carry the step's branch; a handle without steps takes its old side."""
    g = np.load(GOLDEN)
    for name, kind, seed, solver, keep in (("cartpole", "cartpole", 11, "ilqr", 70), ("altro", "cartpole_con", 14, "altro", 70), ("quadrotor", "quadrotor", 15, "ilqr", 16)):
        p = M.build(kind, hip, 70)
        T.set_model_params(p, M.draw_models(kind, 70, seed))
        s = M.SOLVERS[solver](p).solve()
        for k in ("status", "iterations", "cost", "c_max", "iterations_pn"):
            np.testing.assert_array_equal(s.stats[k], g[f"{name}_{k}"], err_msg=f"{name} {k}")
        np.testing.assert_array_equal(T.states(p)[:keep], g[f"{name}_X"], err_msg=name)
        np.testing.assert_array_equal(T.controls(p)[:keep], g[f"{name}_U"], err_msg=name)


# ------------------------------------------------------------------------------------------------ 5. with the other families
def test_own_plants_and_own_steps(hip, oracle):
    kind, B, seed, solver = F.PLANTS_STEPS
    fl, models = F.plants_steps_fleet(oracle)
    assert (fl.stats["status"] == OK).mean() >= 0.9
    p = M.build(kind, hip, B)
    T.set_model_params(p, models)
    T.set_time_steps_batch(p, fl.dt)
    np.testing.assert_array_equal(T.model_params(p), M.params_of(models))        # setting the steps left the plants alone
    s = M.SOLVERS[solver](p).solve()
    assert (s.stats["status"] == OK).mean() >= 0.9
    M.assert_fleet_parity(s, p, fl, unconverged_rtol=1e-4)


def test_own_bounds_and_own_steps(hip, oracle):
    kind, B, seed, solver = F.BOUNDS_STEPS
    fl, a = F.bounds_steps_fleet(oracle)
    assert (fl.stats["status"] == OK).mean() >= 0.9
    p = F.dint_bounds_problem(hip, B)
    T.set_bounds_batch(p, 0, u_max=np.repeat(a[:, None], 2, axis=1), u_min=-np.repeat(a[:, None], 2, axis=1))
    T.set_time_steps_batch(p, fl.dt)
    info = solver_path(p)
    assert info[1] == 0 and info[5] == 0 and (info[7] & 2) == 0, info
    s = M.SOLVERS[solver](p).solve()
    assert (s.stats["status"] == OK).mean() >= 0.9
    M.assert_fleet_parity(s, p, fl, unconverged_rtol=1e-4)


# ------------------------------------------------------------------------------------------------ 6. policy rollout
@pytest.mark.parametrize("B,S,noise", [(70, 3, False), (70, 3, True), (7, 5, True)], ids=["S3", "S3_noise", "S5_B7_noise"])
def test_policy_rollout_steps_each_sample_by_its_trajectory(B, S, noise, hip, oracle):
    """to_policy_rollout (S = 3) and to_policy_rollout_mc with process and measurement noise against the CPU restatement
    (tests/policy_noise_ref.py restate_mc), called once per trajectory on a single-trajectory problem with that trajectory's steps; J from
    the oracle with the samples loaded as trajectories of a problem with those steps (stage costs x dt).  S * B = 210 and 35: neither is a
    multiple of 64; S = 5 packs 12 trajectories per wave, so the 7 trajectories share one wave with idle lanes behind them."""
    import policy_noise_ref as R
    from test_gpu_policy_rollout import RTOL, Stepper
    kind, _, seed = F.POLICY
    kw = dict(options=F.DT_COST)
    dt, _ = F.steps_of(kind, B, seed, True)
    p = M.build(kind, hip, B, **kw)
    T.set_time_steps_batch(p, dt)
    T.iLQRSolver(p).solve()
    Xbar, Ubar = T.states(p), T.controls(p)
    X0s = np.ascontiguousarray(Xbar[:, None, 0, :] + 0.02 * np.random.default_rng(seed).standard_normal((B, S, 4)))
    nz = (lambda b: T.PolicyNoise(2024, sigma_w=0.01, sigma_v=0.01, traj_offset=b)) if noise else (lambda b: None)
    r = T.policy_rollout(p, X0s, trajectories=True, noise=nz(0))
    g = I.gains(p)                                                               # (refresh_gains ran the expansion and the backward pass)
    np.testing.assert_array_equal(r.status, 0)
    worst = {"X": 0.0, "U": 0.0, "dx_max": 0.0, "J": 0.0}
    rel = lambda a, b: (np.abs(a - b).reshape(S, -1).max(axis=1) / np.maximum(1.0, np.abs(b).reshape(S, -1).max(axis=1))).max()
    for b in range(B):
        q1 = F.with_steps(M.build(kind, oracle, 1, b_offset=b, **kw), dt[b], oracle, options=F.DT_COST)
        Xr, Ur, dxr = R.restate_mc(oracle, q1, Xbar[b:b + 1], Ubar[b:b + 1], g["K"][b:b + 1], g["d"][b:b + 1], X0s[b:b + 1], noise=nz(b), Stepper=Stepper)
        qS = F.with_steps(M.build(kind, oracle, S, b_offset=b, **kw), dt[b], oracle, options=F.DT_COST)
        T.initial_states(qS, Xr[0]); T.initial_controls(qS, Ur[0])
        for k, got, want in (("X", r.X[b], Xr[0]), ("U", r.U[b], Ur[0]), ("dx_max", r.dx_max[b], dxr[0]), ("J", r.J[b], T.cost(qS))):
            worst[k] = max(worst[k], rel(got, want))
    print(f"policy rollout on per-trajectory steps (B={B}, S={S}, noise={noise}): " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= RTOL, worst
    # the steps matter here too: on the shared steps the closed-loop states are somewhere else
    T.clear_time_steps_batch(p)
    other = T.policy_rollout(p, X0s, trajectories=True, noise=nz(0), refresh_gains=False)
    # (a law solved for other steps may drive a sample past max_state_value — status != 0, its states not finite from there on: those say
    # "somewhere else" too, the finite ones by how much)
    fin = np.isfinite(other.X).all(axis=(2, 3))
    assert np.all(other.status[~fin] != 0) and fin.any()
    assert np.abs(other.X[fin] - r.X[fin]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 7. refusals
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
        for call in (lambda: T.set_time_steps_batch(p, np.full((p.B, p.N - 1), 0.1)), lambda: T.time_steps(p), lambda: T.clear_time_steps_batch(p)):
            with pytest.raises(T.UnsupportedError, match="per-trajectory time steps are not available for the " + name):
                call()
    # a value that is not finite or not > 0: the first offending trajectory and knot are named, nothing is set
    p = M.build("dint", hip, 5)
    h = T.time_steps(p)
    for v, why in ((np.nan, "is not finite"), (np.inf, "is not finite"), (0.0, "is not > 0"), (-0.1, "is not > 0")):
        bad = h.copy(); bad[3, 7] = v; bad[4, 2] = v
        with pytest.raises(T.ArgumentError, match=f"time step 7 of trajectory 3 {why}"):
            T.set_time_steps_batch(p, bad)
    with pytest.raises(ValueError, match="null pointer"):
        p._call("set_time_steps_batch", None)
    np.testing.assert_array_equal(T.time_steps(p), h)
    assert T.time_steps(p).sum(axis=1).max() == pytest.approx(3.0)
    T.set_time_steps_batch(p, 2.0 * h)                                          # no "must sum to tf - t0" check: twice the horizon is fine
    np.testing.assert_array_equal(T.time_steps(p), 2.0 * h)
    # a solve in flight: like every other handle call
    big = M.build("quadrotor", hip, 256, N=101, tf=5.0)
    s = T.iLQRSolver(big).solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="in flight"):
            T.set_final_times_batch(big, np.full(256, 4.0))
    finally:
        s.wait()
    T.set_final_times_batch(big, np.full(256, 4.0))                             # ... and fine once it has ended


# ------------------------------------------------------------------------------------------------ 8. guard
@pytest.mark.parametrize("case", ["cartpole_coop", "cartpole_altro"])
def test_solves_run_clean_under_the_guard(case, hip, monkeypatch):
    """TRAJOPT_GUARD=1: the per-trajectory array sits between red zones like every other one; an iLQR and an ALTRO solve of the ragged
    fleets run clean and equal the unguarded results bit for bit."""
    out = []
    for guard in ("0", "1"):
        s, p = solve_case(case, True, hip, monkeypatch, guard=guard)
        out.append(results(s, p) + (s.stats["iterations_pn"].copy(), s.stats["c_max"].copy()))
    assert_same(*out)
