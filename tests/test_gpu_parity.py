"""GPU parity: every phase of the hot path computed by libtrajopt_hip.so on the MI355X, through the C-ABI,
against the CPU oracle on identical seeded inputs.  Tolerances: 1e-6 relative (north-star) for solves, much
tighter for single phases; integer outputs (iterations, status, line-search index) bit-exact."""
import ctypes
import json
import math
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

pytestmark = pytest.mark.gpu
G = json.loads((Path(__file__).parent / "golden" / "reference_goldens.json").read_text())


def pair(builder, hip, oracle, **kw):
    return builder(lib=hip, **kw), builder(lib=oracle, **kw)


def perturb_controls(probs, scale, seed=0):
    rng = np.random.default_rng(seed)
    p0 = probs[0]
    U = T.controls(p0) + scale * rng.standard_normal((p0.B, p0.N - 1, p0.m))
    for p in probs:
        T.initial_controls(p, U)


BUILDERS = {
    "cartpole": lambda **kw: configs.cartpole_problem(batch=96, **kw),
    "cartpole_con": lambda **kw: configs.cartpole_problem(batch=70, constrained=True, **kw),
    "quadrotor": lambda **kw: configs.quadrotor_problem(batch=40, N=41, tf=1.0, **kw),
    "quadrotor_con": lambda **kw: configs.quadrotor_problem(batch=40, N=41, tf=1.0, constrained=True, u_norm_max=2.6, **kw),
    "quickstart": lambda **kw: configs.quickstart_problem(batch=3, **kw),
}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_rollout_and_cost(name, hip, oracle):
    ph, po = pair(BUILDERS[name], hip, oracle)
    perturb_controls((ph, po), 0.05)
    T.rollout(ph); T.rollout(po)
    np.testing.assert_allclose(T.states(ph), T.states(po), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(T.cost(ph), T.cost(po), rtol=1e-12)
    np.testing.assert_allclose(T.stage_costs(ph), T.stage_costs(po), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(I.al_cost(ph), I.al_cost(po), rtol=1e-12)
    np.testing.assert_allclose(T.max_violation(ph), T.max_violation(po), rtol=1e-12, atol=1e-14)


def test_G1_golden_rollout_on_gpu(hip):
    model = T.Quadrotor()
    n, m = model.dims()
    x0 = np.zeros(n); x0[:3] = [1, 2, 1]; x0[3] = 1
    xf = np.zeros(n); xf[:3] = [0, 0, 2]; xf[3] = 1
    obj = T.LQRObjective(np.full(n, 0.1), np.full(m, 0.01), np.full(n, 100.0), xf, 51)
    prob = T.Problem(model, obj, x0, 5.0, xf=xf, lib=hip, batch=2)
    T.initial_controls(prob, model.hover_control() + np.array([1, 0, 1, 0]) * 1e-2)
    T.rollout(prob)
    gold = np.array(G["G1_quadrotor_rollout"]["x_final"])
    # the reference's own Float64 output; GPU differs only by FMA contraction (a few ulp over 50 RK4 steps)
    np.testing.assert_allclose(T.states(prob)[1, -1], gold, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_expansion(name, hip, oracle):
    ph, po = pair(BUILDERS[name], hip, oracle)
    perturb_controls((ph, po), 0.05)
    for p in (ph, po):
        T.rollout(p)
        if len(p.constraints):  # non-trivial duals/penalties so every AL branch is exercised
            I.dual_update(p); I.dual_update(p)
        I.expand(p)
    for i in range(len(ph.constraints)):
        lh, mh = I.get_duals(ph, i); lo, mo = I.get_duals(po, i)
        np.testing.assert_allclose(lh, lo, rtol=1e-11, atol=1e-13)
        np.testing.assert_array_equal(mh, mo)
    Ah, Bh = I.dynamics_jacobians(ph); Ao, Bo = I.dynamics_jacobians(po)
    np.testing.assert_allclose(Ah, Ao, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Bh, Bo, rtol=1e-9, atol=1e-11)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for k in Eh:
        np.testing.assert_allclose(Eh[k], Eo[k], rtol=1e-9, atol=1e-10, err_msg=k)
    Fh, Fo = I.discrete_jacobian(ph), I.discrete_jacobian(po)
    np.testing.assert_allclose(Fh, Fo, rtol=1e-9, atol=1e-11)
    gh, Hh = I.cost_gradient_hessian(ph); go, Ho = I.cost_gradient_hessian(po)
    np.testing.assert_allclose(gh, go, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(Hh, Ho, rtol=1e-12, atol=1e-13)
    for i in range(len(ph.constraints)):
        np.testing.assert_allclose(T.evaluate_constraints(ph, i), T.evaluate_constraints(po, i), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(T.constraint_jacobians(ph, i), T.constraint_jacobians(po, i), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_backward_and_forward(name, hip, oracle):
    ph, po = pair(BUILDERS[name], hip, oracle)
    perturb_controls((ph, po), 0.02)
    out = []
    for p in (ph, po):
        T.rollout(p)
        I.expand(p)
        I.backwardpass(p)
        g = I.gains(p)
        ls, J = I.forwardpass(p)
        out.append((g, ls, J, T.states(p), T.controls(p)))
    (gh, lsh, Jh, Xh, Uh), (go, lso, Jo, Xo, Uo) = out
    np.testing.assert_allclose(gh["K"], go["K"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gh["d"], go["d"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gh["dV"], go["dV"], rtol=1e-8)
    np.testing.assert_array_equal(gh["rho"], go["rho"])
    np.testing.assert_array_equal(lsh, lso)
    np.testing.assert_allclose(Jh, Jo, rtol=1e-8)
    np.testing.assert_allclose(Xh, Xo, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(Uh, Uo, rtol=1e-7, atol=1e-9)


def assert_trajectories_close(A, R, rtol, name=""):
    """Relative error of a trajectory in the max norm: max_k,i |A - R| <= rtol * max(1, max_k,i |R|) per trajectory
    (entries that cross zero have no meaningful element-wise relative error).  rtol: scalar or [B]."""
    B = R.shape[0]
    err = np.abs(A - R).reshape(B, -1).max(axis=1)
    scale = np.maximum(1.0, np.abs(R).reshape(B, -1).max(axis=1))
    bad = np.where(~(err <= np.broadcast_to(rtol, (B,)) * scale))[0]
    assert bad.size == 0, f"{name}: trajectories {bad[:8]} off by {(err / scale)[bad[:8]]} (allowed {np.broadcast_to(rtol, (B,))[bad[:8]]})"


def assert_solve_parity(sh, so, ph, po, rtol=1e-6, unconverged_rtol=None):
    """Integer outputs bit-exact; cost / X / U within rtol (north-star 1e-6).  unconverged_rtol: tolerance for the
    trajectories the solver cut off at an iteration limit (they stop on an ill-conditioned iterate, where rounding
    differences are amplified); the converged ones keep rtol."""
    for k in ("iterations", "iterations_outer", "status"):
        np.testing.assert_array_equal(sh.stats[k], so.stats[k], err_msg=k)
    np.testing.assert_allclose(sh.stats["cost"], so.stats["cost"], rtol=rtol)
    np.testing.assert_allclose(sh.stats["c_max"], so.stats["c_max"], rtol=1e-3, atol=1e-9)
    Xh, Xo, Uh, Uo = T.states(ph), T.states(po), T.controls(ph), T.controls(po)
    done = (so.stats["status"] == T.capi.SOLVE_SUCCEEDED) if unconverged_rtol else np.ones(ph.B, bool)
    tol = np.where(done, rtol, unconverged_rtol or rtol)
    assert_trajectories_close(Xh, Xo, tol, "X")
    assert_trajectories_close(Uh, Uo, tol, "U")
    assert sh.total_iterations == so.total_iterations


def test_ilqr_solve_cartpole(hip, oracle):
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=128, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    assert int(sh.stats["iterations"][0]) == 104  # b=0 is the notebook's x0=0 instance (v0.7.1 semantics)
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED)


def test_ilqr_solve_cartpole_legacy_G3(hip):
    """The reference's published iLQR result (84 iterations, J=1.44974) reproduced ON THE GPU."""
    o = T.SolverOptions(lib=hip, cost_dt_scaling=1)
    p = configs.cartpole_problem(batch=2, lib=hip, options=o, integration=T.RK3)
    s = T.iLQRSolver(p).solve()
    g = G["G3_cartpole_ilqr"]
    assert int(s.stats["iterations"][0]) == g["iterations"]
    assert s.stats["cost"][0] == pytest.approx(g["cost"], rel=1e-6)


def test_ilqr_solve_quadrotor(hip, oracle):
    ph, po = pair(lambda **kw: configs.quadrotor_problem(batch=48, N=101, tf=2.5, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)


def test_al_solve_cartpole(hip, oracle):
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=64, constrained=True, **kw), hip, oracle)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    ok = sh.stats["status"] == T.capi.SOLVE_SUCCEEDED
    assert ok.sum() >= 0.8 * ok.size
    assert np.all(sh.stats["c_max"][ok] < 1e-6)


@pytest.mark.parametrize("unit_variants", [True, False])
def test_al_solve_quadrotor_soc(hip, oracle, monkeypatch, unit_variants):
    # C5 shape (Goal@N + ‖u‖₂≤6 SOC) at N=101; constraint_tolerance 1e-4 keeps the solve out of the µ=1e8 tail where
    # any two FP implementations diverge chaotically.  The norm constraint is a "unit SOC": by default the
    # kernel variants specialised for it run (problem_dev.h unit_soc_desc); TRAJOPT_UNIT_SOC=0 takes the general ones.
    if not unit_variants:
        monkeypatch.setenv("TRAJOPT_UNIT_SOC", "0")
    def build(lib):
        o = T.SolverOptions(lib=lib, constraint_tolerance=1e-4)
        return configs.quadrotor_problem(batch=24, N=101, tf=5.0, constrained=True, lib=lib, options=o)
    ph, po = build(hip), build(oracle)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po, rtol=1e-5)
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED)


def test_al_solve_quickstart(hip, oracle):
    ph, po = pair(lambda **kw: configs.quickstart_problem(batch=2, **kw), hip, oracle)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)


@pytest.mark.parametrize("cone", [T.SecondOrderCone(), T.Inequality(), T.Equality(), T.PositiveOrthant(), T.IdentityCone()])
def test_cones(cone, hip, oracle):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((500, 5)) * np.array([1, 1, 1, 1, 3.0])
    b = rng.standard_normal((500, 5))
    np.testing.assert_allclose(T.projection(cone, x, lib=hip), T.projection(cone, x, lib=oracle), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(T.grad_projection(cone, x, lib=hip), T.grad_projection(cone, x, lib=oracle), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(T.hess_projection(cone, x, b, lib=hip), T.hess_projection(cone, x, b, lib=oracle), rtol=1e-12, atol=1e-14)
    if isinstance(cone, T.SecondOrderCone):
        assert T.cone_status(cone, x, lib=hip) == T.cone_status(cone, x, lib=oracle)
        assert T.cone_status(cone, np.array([2, 3, 1, 1.0]), lib=hip) == "outside"      # test/cone_tests.jl:49-54
        assert T.cone_status(cone, np.array([2, 3, 1, -10.0]), lib=hip) == "below"      # :56-60
        assert T.cone_status(cone, np.array([2, 3, 1, 10.0]), lib=hip) == "in"          # :62-66


def test_full_size_C2_vs_oracle(hip, oracle):
    """BASELINE config C2 at full size (Cartpole, N=101, B=1024): EVERY trajectory against the oracle, plus the
    size-independent properties (monotone improvement, dynamic consistency, idempotent rollout)."""
    p = configs.cartpole_problem(batch=1024, lib=hip)
    po = configs.cartpole_problem(batch=1024, lib=oracle)
    T.rollout(p)
    J0 = T.cost(p)
    s, so = T.iLQRSolver(p).solve(), T.iLQRSolver(po).solve()
    # iterations / status bit-exact for all 1024; X, U, J at 1e-6 (the 4 trajectories cut off at MAX_ITERATIONS: 1e-4)
    assert_solve_parity(s, so, p, po, unconverged_rtol=1e-4)
    ok = s.stats["status"] == T.capi.SOLVE_SUCCEEDED
    assert ok.sum() >= 0.99 * ok.size                         # the oracle leaves 4 of 1024 at MAX_ITERATIONS too
    assert set(np.unique(s.stats["status"])) <= {T.capi.SOLVE_SUCCEEDED, T.capi.MAX_ITERATIONS}
    assert np.all(s.stats["cost"] < J0)                       # monotone improvement
    X, U = T.states(p), T.controls(p)
    np.testing.assert_array_equal(X[:, 0], p.x0)              # initial condition untouched
    T.rollout(p)                                              # solution is dynamically consistent: re-simulating the
    X2 = T.states(p)                                          # controls reproduces the states (k_rollout and k_forward are
    np.testing.assert_allclose(X2, X, rtol=1e-9, atol=1e-11)  # separately compiled: last-bit differences only)
    T.rollout(p)
    np.testing.assert_array_equal(T.states(p), X2)            # and the rollout itself is idempotent bit for bit
    np.testing.assert_allclose(T.cost(p), s.stats["cost"], rtol=1e-14)
    assert int(s.stats["iterations"][0]) == 104              # the x0=0 instance
    assert s.total_iterations == int(s.stats["iterations"].sum())
    np.testing.assert_allclose(X[ok, -1, 1], math.pi, atol=0.3)  # swing-up reached


def _subsample_vs_oracle(build, B, oracle, solver):
    """Solve the FULL batch (global trajectories 0..B-1) on the GPU and a deterministic sub-sample — the first two
    tiles and the last tile; inputs are indexed by the global trajectory number, so the oracle can solve just those —
    on the CPU oracle.  Returns (GPU solver, GPU problem, [(index array, oracle solver, oracle problem)])."""
    ph = build(batch=B, b_offset=0)
    sh = solver(ph).solve()
    blocks = []
    for b0, cnt in ((0, 128), (B - 64, 64)):
        po = build(batch=cnt, b_offset=b0, lib=oracle)
        blocks.append((np.arange(b0, b0 + cnt), solver(po).solve(), po))
    return sh, ph, blocks


def elementwise_fraction(A, R, rtol=1e-6, atol=1e-9):
    """share of the entries with |A - R| <= rtol |R| + atol (the element-wise reading of the north-star tolerance; the max-norm
    check of assert_trajectories_close is the one that gates)"""
    return float(np.mean(np.abs(A - R) <= rtol * np.abs(R) + atol))


def test_full_size_C3_vs_oracle(hip, oracle):
    """BASELINE config C3 at its own shape (Quadrotor, N=201, B=4096 = 64 tiles, multi-round residency): ALL 4096 trajectories
    against the oracle (212 k iterations: half a minute on the GPU box's host cores) — integers bit-exact, X / U / J at the
    north-star 1e-6 in the per-trajectory max norm; the element-wise pass fraction (rtol 1e-6, atol 1e-9) is printed next to it."""
    from oracle_binding import set_threads
    ph = configs.quadrotor_problem(N=201, batch=4096, lib=hip)
    sh = T.iLQRSolver(ph).solve()
    po = configs.quadrotor_problem(N=201, batch=4096, lib=oracle)
    set_threads(po, oracle.max_threads())
    so = T.iLQRSolver(po).solve()
    for k in ("iterations", "status"):
        np.testing.assert_array_equal(sh.stats[k], so.stats[k], err_msg=k)
    np.testing.assert_allclose(sh.stats["cost"], so.stats["cost"], rtol=1e-6)
    Xh, Uh, Xo, Uo = T.states(ph), T.controls(ph), T.states(po), T.controls(po)
    assert_trajectories_close(Xh, Xo, 1e-6, "X")
    assert_trajectories_close(Uh, Uo, 1e-6, "U")
    fx, fu = elementwise_fraction(Xh, Xo), elementwise_fraction(Uh, Uo)
    print(f"C3, all 4096 trajectories: element-wise within rtol 1e-6 + atol 1e-9: X {fx:.6f}, U {fu:.6f}; "
          f"worst per-trajectory max-norm error X {np.max(np.abs(Xh - Xo).reshape(4096, -1).max(1) / np.maximum(1, np.abs(Xo).reshape(4096, -1).max(1))):.2e}")
    assert fx >= 0.9999 and fu >= 0.9999
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED)
    assert sh.total_iterations == int(sh.stats["iterations"].sum()) == so.total_iterations


def test_full_size_C5_vs_oracle_subsample(hip, oracle):
    """BASELINE config C5 at its own shape (Quadrotor + GoalConstraint@N + SOC norm cone@1..N-1, N=201, B=8192 =
    128 tiles, first line-search round of 8 step sizes) with the feasible goal (position + velocities) and the default
    constraint_tolerance 1e-6: the sub-sample against the oracle.  AL-iLQR without the projected-Newton polish creeps
    towards 1e-6 over hundreds of iterations at penalty 1e8, which amplifies last-bit differences: the ORACLE AGAINST
    ITSELF with x0 moved by 1-2 ulp separates in 0-2 integer paths of 128 and reaches 1.8e-5 on identical paths
    (tests/test_oracle_sensitivity.py, CPU suite; table in its docstring).  The GPU is held to that measured band: >= 98 %
    identical integer paths, >= 98 % of those within the north-star 1e-6 on X / U / J, none beyond 5e-5, and the same
    outcome class and final violation scale everywhere."""
    from test_oracle_sensitivity import C5_MAX_ERR_SAME_PATH, C5_MIN_IDENTICAL_PATHS, C5_MIN_WITHIN_1E6, c5_compare
    build = lambda **kw: configs.quadrotor_problem(N=201, constrained=True, goal_inds=configs.C5_GOAL_INDS, **{"lib": hip, **kw})
    sh, ph, blocks = _subsample_vs_oracle(build, 8192, oracle, T.ALSolver)
    Xh, Uh = T.states(ph), T.controls(ph)
    same_total, total, errs = 0, 0, []
    for idx, so, po in blocks:
        same, err = c5_compare({k: v[idx] for k, v in sh.stats.items()}, Xh[idx], Uh[idx], so.stats, T.states(po), T.controls(po))
        same_total += int(same.sum()); total += same.size
        errs.append(err)
        # where the paths separated: same problem, same optimum to the accuracy the outer loop reached
        np.testing.assert_allclose(sh.stats["cost"][idx], so.stats["cost"], rtol=2e-3)
        assert np.all(sh.stats["c_max"][idx] < 1e-3) and np.all(so.stats["c_max"] < 1e-3)
    errs = np.concatenate(errs)
    print(f"C5 sub-sample: {same_total}/{total} trajectories with identical iterations/outer/status; on those, X/U/J agree to "
          f"1e-6 for {np.mean(errs <= 1e-6):.1%} (max {errs.max():.2e})")
    assert same_total >= C5_MIN_IDENTICAL_PATHS * total
    assert np.mean(errs <= 1e-6) >= C5_MIN_WITHIN_1E6 and errs.max() <= C5_MAX_ERR_SAME_PATH
    ok = sh.stats["status"] == T.capi.SOLVE_SUCCEEDED
    assert np.all(sh.stats["c_max"][ok] < 1e-6)
    assert set(np.unique(sh.stats["status"])) <= {T.capi.SOLVE_SUCCEEDED, T.capi.MAX_ITERATIONS, T.capi.MAX_ITERATIONS_OUTER}


def test_G4_quadrotor_zigzag_on_gpu(hip, oracle, monkeypatch):
    """The reference's Quadrotor zig-zag (examples/Quadrotor.ipynb cells 10-22, golden G4_quadrotor_altro: 90
    iterations, J = 0.29928, violation 7.6e-10) solved on the GPU: per-knot waypoint costs + control bounds, AL-iLQR.
    Sanity against the notebook (the S4 pin SURVEY §8c prescribes: cost to 1 %, feasible to 1e-6) and parity against the
    oracle.  The start — 1/20 of the hover thrust, 20 m to fly — makes the solve chaotic in the start position: moved by
    1e-2 m the ORACLE itself needs 58 ... 591 iterations instead of 85, so only the notebook's own start is compared, and the
    oracle's path is followed step for step only as long as no line-search decision sits within rounding of its threshold
    (round 3: a 2e-14 difference in J between the two forward kernels was enough for 68 instead of 85 iterations).  What must
    hold exactly: the one-wave kernel and the per-step choice between the two forward kernels give the SAME solve, bit for bit."""
    g = G["G4_quadrotor_altro"]
    runs = {}
    for mode in ("0", "auto"):
        if mode == "0":
            monkeypatch.setenv("TRAJOPT_FWD2", "0")
        else:
            monkeypatch.delenv("TRAJOPT_FWD2", raising=False)
        ph, wpts, times = configs.quadrotor_zigzag_problem(lib=hip, batch=5)   # the notebook's single start, in every lane
        runs[mode] = (T.ALSolver(ph).solve(), ph)
    (s0, p0), (sh, ph) = runs["0"], runs["auto"]
    for k in ("iterations", "iterations_outer", "status", "cost", "c_max"):
        np.testing.assert_array_equal(s0.stats[k], sh.stats[k], err_msg=k)
    np.testing.assert_array_equal(T.states(p0), T.states(ph))
    np.testing.assert_array_equal(T.controls(p0), T.controls(ph))
    po, _, _ = configs.quadrotor_zigzag_problem(lib=oracle, batch=5)
    so = T.ALSolver(po).solve()
    assert int(sh.stats["status"][0]) == T.capi.SOLVE_SUCCEEDED
    assert sh.stats["c_max"][0] < 1e-6
    assert sh.stats["cost"][0] == pytest.approx(g["cost"], rel=1e-2)
    assert abs(int(sh.stats["iterations"][0]) - g["iterations"]) <= g["iterations"] // 3
    Xh = T.states(ph)
    for r, k in zip(wpts[:2], times[:2]):
        assert np.linalg.norm(Xh[0, k - 1, :3] - r) < 0.6
    assert np.linalg.norm(Xh[0, -1, :3] - wpts[2]) < 5e-3
    np.testing.assert_array_equal(sh.stats["iterations"], sh.stats["iterations"][0])   # identical lanes stay identical
    print("zig-zag: GPU", int(sh.stats["iterations"][0]), "iterations, oracle", int(so.stats["iterations"][0]))
    if np.array_equal(sh.stats["iterations"], so.stats["iterations"]):
        for k in ("iterations_outer", "status"):
            np.testing.assert_array_equal(sh.stats[k], so.stats[k], err_msg=k)
        np.testing.assert_allclose(sh.stats["cost"], so.stats["cost"], rtol=1e-6)
        assert_trajectories_close(Xh, T.states(po), 1e-6, "X")
        assert_trajectories_close(T.controls(ph), T.controls(po), 1e-6, "U")
    else:
        np.testing.assert_allclose(sh.stats["cost"], so.stats["cost"], rtol=1e-2)


@pytest.mark.parametrize("rot", ["mrp", "rp"])
def test_three_parameter_attitude_quadrotor_on_gpu(rot, hip, oracle):
    """RigidBody{MRP} / RigidBody{RodriguesParam} (src/lie_costs.jl:1-3): the Quadrotor with a three-parameter
    attitude (n = ne = 12) and ErrorQuadratic{Rot}.  Every phase against the oracle (whose closed forms are pinned by finite
    differences in tests/test_oracle_rotations.py; the GPU differentiates the same maps with dual numbers), then full iLQR
    and AL solves."""
    def build(lib, constrained=False, batch=24, N=41, tf=2.0):
        model = T.Quadrotor(rotation=rot)
        n, m = model.dims()
        th = math.radians(70.0) / 2
        xf = model.build_state([1.0, 1.5, 0.5], [math.cos(th), 0.0, 0.0, math.sin(th)])
        Qe = np.r_[np.ones(3), 0.5 * np.ones(3), 0.1 * np.ones(6)]
        stage = T.ErrorQuadratic(model, Qe, np.full(m, 1e-2), xf, model.hover_control())
        term = T.ErrorQuadratic(model, 100 * Qe, np.full(m, 1e-2), xf, model.hover_control(), terminal=True)
        cons = T.ConstraintList(n, m, N)
        if constrained:
            T.add_constraint(cons, T.BoundConstraint(n, m, u_min=0.0, u_max=2.2), range(1, N))
            T.add_constraint(cons, T.GoalConstraint(xf, [1, 2, 3, 7, 8, 9, 10, 11, 12]), N)
        prob = T.Problem(model, T.Objective(stage, term, N), np.zeros(n), tf, xf=xf, constraints=cons, batch=batch, lib=lib)
        rng = np.random.default_rng(11)
        x0 = np.zeros((batch, n)); x0[:, :3] = rng.uniform(-0.5, 0.5, (batch, 3)); x0[:, 3:6] = 0.1 * rng.standard_normal((batch, 3))
        prob.set_initial_state(x0)
        T.initial_controls(prob, model.hover_control())
        return prob

    # phases on a 1 s open-loop rollout: uncontrolled, the perturbed quadrotor tumbles, and over 2 s some trajectories pass through
    # 180 deg — where a RodriguesParam is infinite (oracle and GPU alike: g ~ 1e47, NaN Jacobians) and an MRP flips to its shadow set
    ph, po = build(hip, tf=1.0), build(oracle, tf=1.0)
    perturb_controls((ph, po), 0.02)
    T.rollout(ph); T.rollout(po)
    assert np.all(np.isfinite(T.states(po))) and np.abs(T.states(po)[:, :, 3:6]).max() < 1.0
    np.testing.assert_allclose(T.states(ph), T.states(po), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(T.cost(ph), T.cost(po), rtol=1e-12)
    np.testing.assert_allclose(I.discrete_jacobian(ph), I.discrete_jacobian(po), rtol=1e-9, atol=1e-11)
    gh, Hh = I.cost_gradient_hessian(ph)
    go, Ho = I.cost_gradient_hessian(po)
    np.testing.assert_allclose(gh, go, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(Hh, Ho, rtol=1e-9, atol=1e-11)
    for p in (ph, po):
        I.expand(p); I.backwardpass(p)
    (Ah, Bh), (Ao, Bo) = I.dynamics_jacobians(ph), I.dynamics_jacobians(po)
    np.testing.assert_allclose(Ah, Ao, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Bh, Bo, rtol=1e-9, atol=1e-11)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for k in Eh:
        np.testing.assert_allclose(Eh[k], Eo[k], rtol=1e-9, atol=1e-10, err_msg=k)
    kh, ko = I.gains(ph), I.gains(po)
    np.testing.assert_array_equal(kh["rho"], ko["rho"])
    np.testing.assert_allclose(kh["K"], ko["K"], rtol=1e-6, atol=1e-8)   # 40 knots of Riccati recursion on 1e-9 expansions
    np.testing.assert_allclose(kh["d"], ko["d"], rtol=1e-6, atol=1e-8)
    lh, Jh = I.forwardpass(ph)
    lo, Jo = I.forwardpass(po)
    np.testing.assert_array_equal(lh, lo)
    np.testing.assert_allclose(Jh, Jo, rtol=1e-8)
    ph, po = build(hip), build(oracle)
    assert_solve_parity(T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve(), ph, po)
    ph, po = build(hip, constrained=True), build(oracle, constrained=True)
    sh, so = T.ALSolver(ph, constraint_tolerance=1e-5).solve(), T.ALSolver(po, constraint_tolerance=1e-5).solve()
    assert_solve_parity(sh, so, ph, po)
    assert np.all(sh.stats["c_max"] < 1e-5)


# ---------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_ragged_batch_sizes(B, hip, oracle):
    """Batches that do not fill a 64-trajectory tile / an 8-trajectory column group."""
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=B, N=31, tf=1.5, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph, iterations=25).solve(), T.iLQRSolver(po, iterations=25).solve()
    assert_solve_parity(sh, so, ph, po)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_double_integrator_models(D, hip, oracle):
    def build(lib):
        model = T.DoubleIntegrator(1.3, D)
        n, m = model.dims()
        xf = np.concatenate([np.arange(1, D + 1, dtype=float), np.zeros(D)])
        obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 10.0 * np.ones(n), xf, 16)
        cons = T.ConstraintList(n, m, 16)
        T.add_constraint(cons, T.BoundConstraint(n, m, u_min=-2.0, u_max=2.0), range(1, 16))
        T.add_constraint(cons, T.GoalConstraint(xf), 16)
        p = T.Problem(model, obj, np.zeros(n), 2.0, xf=xf, constraints=cons, batch=5, lib=lib,
                      options=T.SolverOptions(lib=lib, constraint_tolerance=1e-5))
        p.set_initial_state(np.linspace(-0.5, 0.5, 5)[:, None] * np.ones((5, n)))
        return p
    ph, po = build(hip), build(oracle)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)


def test_minimal_horizon_and_nonuniform_dt(hip, oracle):
    """N=2 (a single step) and a non-uniform dt vector (test/problems_tests.jl:78-85)."""
    def build(lib, N, dt):
        model = T.Cartpole()
        obj = T.LQRObjective(np.full(4, 1e-2), np.full(1, 1e-1), np.full(4, 10.0), np.array([0, np.pi, 0, 0.0]), N)
        p = T.Problem(model, obj, np.zeros(4), float(np.sum(dt)), dt=dt, batch=3, lib=lib)
        T.initial_controls(p, np.array([0.3]))
        return p
    for N, dt in [(2, np.array([0.1])), (6, np.array([0.05, 0.1, 0.02, 0.2, 0.13]))]:
        ph, po = build(hip, N, dt), build(oracle, N, dt)
        T.rollout(ph); T.rollout(po)
        np.testing.assert_allclose(T.states(ph), T.states(po), rtol=1e-12, atol=1e-14)
        sh, so = T.iLQRSolver(ph, iterations=10).solve(), T.iLQRSolver(po, iterations=10).solve()
        assert_solve_parity(sh, so, ph, po)


@pytest.mark.parametrize("full_newton", [0, 1])
def test_every_constraint_kind_and_dense_cost(full_newton, hip, oracle):
    """All six constraint kinds + QuadraticCost with a cross term H + per-knot distinct costs in one problem; with
    al_full_newton = 1 the expansion also carries the constraint curvature (circle, sphere, collision, quadratic norm,
    QuatVecEq) — the cost blocks and the solves must still match the oracle."""
    rng = np.random.default_rng(11)

    def build(lib):
        model = T.Quadrotor(); n, m = model.dims(); N = 12
        xf = np.zeros(n); xf[:3] = [0.5, 0.3, 0.8]; xf[3] = 1
        Q = np.diag(np.r_[np.ones(3), np.zeros(4), 0.1 * np.ones(6)]); Q[0, 1] = Q[1, 0] = 0.05
        R = 0.02 * np.eye(m) + 0.001
        H = 1e-3 * np.arange(m * n, dtype=float).reshape(m, n) / (m * n)
        u0 = model.hover_control()
        dense = T.QuadraticCost(Q, R, H, -Q @ xf, -R @ u0, 0.3)
        diag = T.LQRCost(np.diag(Q), np.diag(R), xf, u0)
        term = T.LQRCost(50 * np.diag(Q), np.diag(R), xf, u0, terminal=True)
        obj = T.Objective([dense if k % 2 else diag for k in range(N - 1)] + [term])
        cons = T.ConstraintList(n, m, N)
        T.add_constraint(cons, T.GoalConstraint(xf, [1, 2, 3]), N)
        T.add_constraint(cons, T.NormConstraint(n, m, 3.5, T.SecondOrderCone(), "control"), range(1, N))
        T.add_constraint(cons, T.NormConstraint(n, m, 4.0, T.Inequality(), [8, 9, 10]), range(1, N + 1))
        T.add_constraint(cons, T.BoundConstraint(n, m, u_min=0.0, u_max=2.5, x_max=np.r_[3.0, np.full(12, np.inf)]), range(1, N))
        T.add_constraint(cons, T.CircleConstraint(n, [0.25], [0.1], [0.05]), range(2, N))
        T.add_constraint(cons, T.SphereConstraint(n, [0.4], [0.4], [0.2], [0.05]), range(2, N))
        A = rng.standard_normal((2, 3)); b = np.array([5.0, 6.0])
        T.add_constraint(cons, T.LinearConstraint(n, m, A, b, T.Inequality(), [1, 2, 14]), range(1, N))
        T.add_constraint(cons, T.CollisionConstraint(n, [1, 2, 3], [8, 9, 10], 0.02), range(2, N + 1))
        T.add_constraint(cons, T.QuatVecEq(n, m, xf[3:7]), N)
        x0 = np.zeros(n); x0[3] = 1
        p = T.Problem(model, obj, x0, 1.1, xf=xf, constraints=cons, batch=6, lib=lib,
                      options=T.SolverOptions(lib=lib, constraint_tolerance=1e-4, iterations_outer=6, al_full_newton=full_newton))
        T.initial_controls(p, u0)
        return p
    rng = np.random.default_rng(11); ph = build(hip)
    rng = np.random.default_rng(11); po = build(oracle)
    for p in (ph, po):
        T.rollout(p); I.dual_update(p); I.expand(p)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for k in Eh:
        np.testing.assert_allclose(Eh[k], Eo[k], rtol=1e-9, atol=1e-10, err_msg=k)
    for i in range(len(ph.constraints)):
        np.testing.assert_allclose(T.evaluate_constraints(ph, i), T.evaluate_constraints(po, i), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(T.constraint_jacobians(ph, i), T.constraint_jacobians(po, i), rtol=1e-12, atol=1e-13)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po, rtol=1e-5)


def test_resolve_after_goal_change(hip, oracle):
    """MPC-style reuse: set_goal_state! between solves (src/problem.jl:294-310) and warm start from the last solution."""
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=4, N=41, tf=2.0, constrained=True, **kw), hip, oracle)
    for p in (ph, po):
        T.ALSolver(p, iterations_outer=3).solve()
        T.set_goal_state(p, np.array([0.2, np.pi, 0, 0.0]))
    sh, so = T.ALSolver(ph, iterations_outer=3).solve(), T.ALSolver(po, iterations_outer=3).solve()
    assert_solve_parity(sh, so, ph, po, rtol=1e-5)


@pytest.mark.parametrize("t1", [1, 3])
def test_line_search_round_schedule(t1, hip, oracle, monkeypatch):
    """The concurrent line search must equal sequential backtracking for ANY round schedule: with a first round of 1
    or 3 step sizes the later rounds run on the compacted list with geometrically growing widths (throughput regime)."""
    monkeypatch.setenv("TRAJOPT_LS_CANDIDATES", str(t1))
    monkeypatch.setenv("TRAJOPT_LS_DEEP", "0")
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=96, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=40, constrained=True, **kw), hip, oracle)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    # the Quadrotor path (gains staged through LDS, k_accept): narrow rounds continued inside the kernel ...
    ph, po = pair(lambda **kw: configs.quadrotor_problem(batch=37, N=61, tf=1.5, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph, iterations=40).solve(), T.iLQRSolver(po, iterations=40).solve()
    assert_solve_parity(sh, so, ph, po)
    # ... and the deep shape (the whole search depth in one round: 20 step sizes x 3 trajectories per wave, the last wave
    # reaching past the batch), which the solve loop switches to once the active trajectories fit the chip
    monkeypatch.delenv("TRAJOPT_LS_DEEP")
    ph, po = pair(lambda **kw: configs.quadrotor_problem(batch=37, N=61, tf=1.5, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph, iterations=40).solve(), T.iLQRSolver(po, iterations=40).solve()
    assert_solve_parity(sh, so, ph, po)


def test_long_horizons(hip, oracle):
    """Horizons well past the BASELINE shapes (index arithmetic, per-knot buffers, double-buffered gains): Cartpole N=1501,
    constrained Cartpole N=801, Quadrotor N=601 — a few iterations each, batches that are not multiples of anything."""
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=5, N=1501, tf=15.0, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph, iterations=12).solve(), T.iLQRSolver(po, iterations=12).solve()
    assert_solve_parity(sh, so, ph, po, unconverged_rtol=1e-4)
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=3, N=801, tf=8.0, constrained=True, **kw), hip, oracle)
    kw = dict(iterations=8, iterations_outer=2, iterations_total=16)
    sh, so = T.ALSolver(ph, **kw).solve(), T.ALSolver(po, **kw).solve()
    assert_solve_parity(sh, so, ph, po, unconverged_rtol=1e-4)
    ph, po = pair(lambda **kw: configs.quadrotor_problem(batch=3, N=601, tf=15.0, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph, iterations=6).solve(), T.iLQRSolver(po, iterations=6).solve()
    assert_solve_parity(sh, so, ph, po, unconverged_rtol=1e-4)


@pytest.mark.parametrize("width", [8, 4])
def test_forward_wave_shape_is_invisible_constrained_quadrotor(width, hip, monkeypatch):
    """The forward-wave shape (step sizes per round x trajectories per wave) must not change a single bit: the constrained
    Quadrotor batch stepped through the phase API with 16 step sizes per round and with `width`.  This is the scenario that
    exposed the compiler's spill-placement hazard: with >= 6 candidates of a trajectory in lanes >= 40 the
    second round of the line search ran with a corrupted step size, 40 iterations into the solve."""
    monkeypatch.setenv("TRAJOPT_LS_DEEP", "0")
    probs = []
    for cw in (16, width):
        monkeypatch.setenv("TRAJOPT_LS_CANDIDATES", str(cw))
        o = T.SolverOptions(lib=hip, constraint_tolerance=1e-4)
        p = configs.quadrotor_problem(batch=24, N=101, tf=5.0, constrained=True, lib=hip, options=o)
        T.rollout(p)
        probs.append(p)
    deep_rounds = 0
    for it in range(48):
        out = []
        for p in probs:
            if it % 15 == 14:
                I.dual_update(p)
            I.expand(p); I.backwardpass(p)
            ls, J = I.forwardpass(p)
            out.append((ls, J, T.states(p)))
        (l0, J0, X0), (l1, J1, X1) = out
        np.testing.assert_array_equal(l0, l1, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(J0, J1, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(X0, X1, err_msg=f"iteration {it}")
        deep_rounds += int((l0 >= width).sum())
    assert deep_rounds > 20  # the narrow shape really went through second and third rounds


def test_lane_backward_on_small_models(hip, oracle, monkeypatch):
    """The one-lane-per-trajectory backward pass (lane-layout expansion; default only for batches that would stack the
    cooperative waves three deep) forced on small batches: expansion getters, gains, and full solves for m = 1
    (Cartpole, constrained and not, a batch that is not a multiple of 64) and m = 2 (2-D double integrator with bounds)."""
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")
    ph, po = pair(BUILDERS["cartpole_con"], hip, oracle)
    perturb_controls((ph, po), 0.02)
    for p in (ph, po):
        T.rollout(p); I.dual_update(p); I.expand(p); I.backwardpass(p)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for k in Eh:
        np.testing.assert_allclose(Eh[k], Eo[k], rtol=1e-9, atol=1e-10, err_msg=k)
    Ah, Bh = I.dynamics_jacobians(ph)
    Ao, Bo = I.dynamics_jacobians(po)
    np.testing.assert_allclose(Ah, Ao, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(Bh, Bo, rtol=1e-10, atol=1e-12)
    gh, go = I.gains(ph), I.gains(po)
    np.testing.assert_array_equal(gh["rho"], go["rho"])
    np.testing.assert_allclose(gh["K"], go["K"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gh["d"], go["d"], rtol=1e-7, atol=1e-9)
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=70, **kw), hip, oracle)
    assert_solve_parity(T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve(), ph, po)
    ph, po = pair(BUILDERS["cartpole_con"], hip, oracle)
    assert_solve_parity(T.ALSolver(ph).solve(), T.ALSolver(po).solve(), ph, po)
    def di2(lib):
        model = T.DoubleIntegrator(0.8, 2)
        n, m = model.dims()
        xf = np.array([1.0, -2.0, 0.0, 0.0])
        obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 10.0 * np.ones(n), xf, 21)
        cons = T.ConstraintList(n, m, 21)
        T.add_constraint(cons, T.BoundConstraint(n, m, u_min=-1.5, u_max=1.5), range(1, 21))
        T.add_constraint(cons, T.GoalConstraint(xf), 21)
        p = T.Problem(model, obj, np.zeros(n), 2.0, xf=xf, constraints=cons, batch=9, lib=lib,
                      options=T.SolverOptions(lib=lib, constraint_tolerance=1e-5))
        p.set_initial_state(np.linspace(-0.5, 0.5, 9)[:, None] * np.ones((9, n)))
        return p
    ph, po = di2(hip), di2(oracle)
    assert_solve_parity(T.ALSolver(ph).solve(), T.ALSolver(po).solve(), ph, po)


def test_lane_expansion_matches_column_expansion(hip, oracle, monkeypatch):
    """k_expand_lane (one lane per (trajectory, knot), every column of [A B] from ONE pass of the RK stages in chunk-mode dual
    numbers) against the column-per-lane kernel it replaces for the lane layout (TRAJOPT_EXPAND_LANE=0) and against the
    oracle's analytic chain rule: Cartpole (diagonal cost, bounds + goal: VAR 2), the quickstart double integrator (circle +
    SOC + bounds: VAR 7, a ragged batch) and a dense QuadraticCost with a cross term (VAR 1)."""
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")

    def dense(lib):
        model = T.DoubleIntegrator(1.3, 2)
        n, m, N = 4, 2, 17
        rng = np.random.default_rng(5)
        A = rng.standard_normal((n, n)); Q = A @ A.T + n * np.eye(n)
        Bm = rng.standard_normal((m, m)); R = Bm @ Bm.T + m * np.eye(m)
        H = 0.1 * rng.standard_normal((m, n))
        stage = T.QuadraticCost(Q, R, H, rng.standard_normal(n), rng.standard_normal(m), 0.3)
        term = T.QuadraticCost(3 * Q, R, None, rng.standard_normal(n), None, 0.1, terminal=True)
        p = T.Problem(model, T.Objective(stage, term, N), np.zeros(n), 1.6, batch=67, lib=lib)
        p.set_initial_state(rng.standard_normal((67, n)))
        return p

    for name, build in (("cartpole_con", BUILDERS["cartpole_con"]), ("quickstart", lambda **kw: configs.quickstart_problem(batch=67, **kw)), ("dense", None)):
        res = {}
        for mode in ("1", "0", "oracle"):
            monkeypatch.setenv("TRAJOPT_EXPAND_LANE", "1" if mode == "oracle" else mode)
            lib = oracle if mode == "oracle" else hip
            p = dense(lib) if build is None else build(lib=lib)
            perturb_controls((p,), 0.05, seed=3)
            T.rollout(p)
            if len(p.constraints):
                I.dual_update(p)
            I.expand(p)
            I.backwardpass(p)
            res[mode] = (I.dynamics_jacobians(p), I.cost_expansion(p), I.gains(p))
        (A1, B1), E1, g1 = res["1"]
        (A0, B0), E0, g0 = res["0"]
        (Ao, Bo), Eo, go = res["oracle"]
        # same operations per derivative component as the single-direction dual numbers: identical up to FMA contraction
        np.testing.assert_allclose(A1, A0, rtol=1e-14, atol=1e-15, err_msg=name)
        np.testing.assert_allclose(B1, B0, rtol=1e-14, atol=1e-15, err_msg=name)
        for k in E1:
            np.testing.assert_allclose(E1[k], E0[k], rtol=1e-14, atol=1e-15, err_msg=f"{name} {k}")
            np.testing.assert_allclose(E1[k], Eo[k], rtol=1e-9, atol=1e-10, err_msg=f"{name} {k} vs oracle")
        np.testing.assert_allclose(A1, Ao, rtol=1e-10, atol=1e-12, err_msg=name)
        np.testing.assert_allclose(B1, Bo, rtol=1e-10, atol=1e-12, err_msg=name)
        np.testing.assert_array_equal(g1["rho"], go["rho"])
        np.testing.assert_allclose(g1["K"], go["K"], rtol=1e-7, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(g1["d"], go["d"], rtol=1e-7, atol=1e-9, err_msg=name)


def test_fused_lane_solve_matches_split_kernels(hip, monkeypatch):
    """k_expand_backward_lane (the solve loop of the lane path: every knot expanded in the registers of the lane that runs
    the Riccati recursion, no expansion arrays in memory) against k_expand_lane + k_backward_lane (TRAJOPT_FUSED_LANE=0):
    same operations in the same order, so iterations / status are identical and the trajectories agree to 1e-6 — with and
    without active-list compaction (TRAJOPT_COMPACT), on the unconstrained Cartpole (a ragged batch), AL with bounds + goal,
    and the quickstart problem (circle + SOC: VAR 7)."""
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")
    cases = [(lambda: configs.cartpole_problem(batch=130, lib=hip), T.iLQRSolver, {}),
             (lambda: BUILDERS["cartpole_con"](lib=hip), T.ALSolver, {}),
             (lambda: configs.quickstart_problem(batch=67, lib=hip), T.ALSolver, {"u0": np.array([0.1, 0.0])})]
    for build, Solver, kw in cases:
        out = []
        for fused, compact in (("1", "1"), ("0", "0"), ("1", "0")):
            monkeypatch.setenv("TRAJOPT_FUSED_LANE", fused)
            monkeypatch.setenv("TRAJOPT_COMPACT", compact)
            p = build()
            if "u0" in kw:
                T.initial_controls(p, kw["u0"])
            s = Solver(p).solve()
            out.append(({k: v.copy() for k, v in s.stats.items()}, T.states(p), T.controls(p), s.batch_steps))
        (s1, X1, U1, n1), (s0, X0, U0, n0), (s2, X2, U2, n2) = out
        # compaction only changes which lane works on which trajectory: bit-identical to the same kernel without it
        assert n1 == n2
        for k in s1:
            np.testing.assert_array_equal(s1[k], s2[k], err_msg=f"compaction: {k}")
        np.testing.assert_array_equal(X1, X2)
        np.testing.assert_array_equal(U1, U2)
        assert n1 == n0
        for k in ("iterations", "iterations_outer", "status"):
            np.testing.assert_array_equal(s1[k], s0[k], err_msg=k)
        # same operations in the same order, but two kernels are two compilations: FMA contraction differs in places, and a
        # hundred iterations carry a last-bit difference to 1e-7 (measured 4e-7 on the Cartpole) — the north-star 1e-6 holds
        assert_trajectories_close(X1, X0, 1e-6, "X")
        assert_trajectories_close(U1, U0, 1e-6, "U")
        np.testing.assert_allclose(s1["cost"], s0["cost"], rtol=1e-6)


def test_compaction_on_the_mfma_path_is_bit_identical(hip, monkeypatch):
    """Active-list compaction on the Quadrotor (MFMA) path — k_expand, k_backward_mfma and k_forward take their trajectories
    from the list of the still-active ones — changes which wave works on which trajectory and nothing else: iLQR and AL
    solves with and without it (TRAJOPT_COMPACT) are bit-identical, on a batch that drains unevenly (70 trajectories: ragged
    tiles, start positions spread over 2 m) and, for the small models forced onto the MFMA path, with write-through."""
    cases = [(lambda: configs.quadrotor_problem(batch=70, N=41, tf=1.0, lib=hip), T.iLQRSolver, None),
             (lambda: configs.quadrotor_problem(batch=70, N=41, tf=1.0, constrained=True, u_norm_max=2.6, lib=hip), T.ALSolver, None),
             (lambda: BUILDERS["cartpole_con"](lib=hip), T.ALSolver, "mfma")]
    for build, Solver, bwd in cases:
        if bwd:
            monkeypatch.setenv("TRAJOPT_BACKWARD", bwd)
        out = []
        for compact in ("1", "0"):
            monkeypatch.setenv("TRAJOPT_COMPACT", compact)
            p = build()
            s = Solver(p).solve()
            out.append(({k: v.copy() for k, v in s.stats.items()}, T.states(p), T.controls(p), s.batch_steps))
        (s1, X1, U1, n1), (s0, X0, U0, n0) = out
        assert n1 == n0 and len(set(s1["iterations"])) > 3
        for k in s1:
            np.testing.assert_array_equal(s1[k], s0[k], err_msg=k)
        np.testing.assert_array_equal(X1, X0)
        np.testing.assert_array_equal(U1, U0)
        if bwd:
            monkeypatch.delenv("TRAJOPT_BACKWARD")


def test_fused_cooperative_pass_matches_split_kernels(hip, oracle, monkeypatch):
    """k_expand_backward_coop (small batches of the small models, diagonal cost blocks: a second wave of the workgroup expands the
    knots the Riccati wave is about to consume, through an LDS ring — no expansion arrays in memory) against k_expand +
    k_backward_coop (TRAJOPT_FUSED_COOP=0) and against the oracle: gains of one pass, then full solves — Cartpole iLQR on a
    ragged batch, AL with bounds + goal, a 2-D double integrator with bounds (m = 2), and a non-uniform time grid.  None of these
    batches restarts a backward pass (rho stays 0 on the oracle, the rough start below included): the restart of the whole workgroup and
    the failed passes are held to the oracle by tests/test_gpu_failure_paths.py."""
    def di2(lib):
        model = T.DoubleIntegrator(0.8, 2)
        n, m = model.dims()
        xf = np.array([1.0, -2.0, 0.0, 0.0])
        obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 10.0 * np.ones(n), xf, 21)
        cons = T.ConstraintList(n, m, 21)
        T.add_constraint(cons, T.BoundConstraint(n, m, u_min=-1.5, u_max=1.5), range(1, 21))
        T.add_constraint(cons, T.GoalConstraint(xf), 21)
        dt = np.linspace(0.05, 0.15, 20); dt *= 2.0 / dt.sum()
        p = T.Problem(model, obj, np.zeros(n), 2.0, xf=xf, constraints=cons, batch=9, lib=lib, dt=dt,
                      options=T.SolverOptions(lib=lib, constraint_tolerance=1e-5))
        p.set_initial_state(np.linspace(-0.5, 0.5, 9)[:, None] * np.ones((9, n)))
        return p

    # one backward pass: gains, rho, predicted decrease — the fused kernel only runs inside solves, so compare after ONE iteration
    cases = [(lambda lib: configs.cartpole_problem(batch=130, lib=lib), T.iLQRSolver),
             (lambda lib: BUILDERS["cartpole_con"](lib=lib), T.ALSolver),
             (di2, T.ALSolver)]
    for build, Solver in cases:
        res = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("TRAJOPT_FUSED_COOP", mode)
            p = build(hip)
            s = Solver(p).solve()
            res[mode] = ({k: v.copy() for k, v in s.stats.items()}, T.states(p), T.controls(p), s.batch_steps)
        po = build(oracle)
        so = Solver(po).solve()
        (s1, X1, U1, n1), (s0, X0, U0, n0) = res["1"], res["0"]
        assert n1 == n0
        for k in ("iterations", "iterations_outer", "status"):
            np.testing.assert_array_equal(s1[k], s0[k], err_msg=k)
            np.testing.assert_array_equal(s1[k], so.stats[k], err_msg=k + " vs oracle")
        assert_trajectories_close(X1, X0, 1e-6, "X")
        assert_trajectories_close(U1, U0, 1e-6, "U")
        assert_trajectories_close(X1, T.states(po), 1e-6, "X vs oracle")
        assert_trajectories_close(U1, T.controls(po), 1e-6, "U vs oracle")
        np.testing.assert_allclose(s1["cost"], so.stats["cost"], rtol=1e-6)
    monkeypatch.setenv("TRAJOPT_FUSED_COOP", "1")
    # a rough start (controls perturbed by 1.0), three iterations: deeper line searches, no restart (rho is 0 throughout, compared exactly)
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=70, **kw), hip, oracle)
    perturb_controls((ph, po), 1.0, seed=5)
    sh, so = T.iLQRSolver(ph, iterations=3).solve(), T.iLQRSolver(po, iterations=3).solve()
    gh, go = I.gains(ph), I.gains(po)
    np.testing.assert_array_equal(gh["rho"], go["rho"])
    assert_solve_parity(sh, so, ph, po)


def test_large_batch_compaction_two_launch_path(hip, monkeypatch):
    """Batches beyond 16 384 trajectories build their active lists with the two-launch compaction (k_compact_count /
    k_compact_write, index order): 20 000 Cartpole trajectories (ragged: 313 tiles, the last one partly empty) on the fused lane
    path, 40 iterations so that part of the batch has converged and the lists have holes — bit-identical to the same solve
    without compaction.  (Unconstrained batches below ~20 000 default to the scan + cooperative kernels: the lane path is forced.)"""
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")
    out = []
    for compact in ("1", "0"):
        monkeypatch.setenv("TRAJOPT_COMPACT", compact)
        p = configs.cartpole_problem(batch=20000, N=41, tf=2.0, lib=hip)
        s = T.iLQRSolver(p, iterations=40).solve()
        out.append(({k: v.copy() for k, v in s.stats.items()}, T.states(p), T.controls(p), s.batch_steps))
    (s1, X1, U1, n1), (s0, X0, U0, n0) = out
    assert n1 == n0 and 0 < np.mean(s1["status"] == T.capi.SOLVE_SUCCEEDED) < 1 or len(set(s1["iterations"])) > 5
    for k in s1:
        np.testing.assert_array_equal(s1[k], s0[k], err_msg=k)
    np.testing.assert_array_equal(X1, X0)
    np.testing.assert_array_equal(U1, U0)


def test_mfma_backward_on_small_models(hip, oracle, monkeypatch):
    """The MFMA backward pass (one wave per trajectory, tangent-matrix expansion, compact and full cost blocks) is generic
    in the model; the small models default to the cooperative kernel, so force it: m = 1 / ne = 4 (Cartpole) and
    ne = 6 -> padded to 8, m = 3 (3-D double integrator, bounds + goal)."""
    monkeypatch.setenv("TRAJOPT_BACKWARD", "mfma")
    ph, po = pair(BUILDERS["cartpole_con"], hip, oracle)
    perturb_controls((ph, po), 0.02)
    for p in (ph, po):
        T.rollout(p); I.dual_update(p); I.expand(p); I.backwardpass(p)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for k in Eh:
        np.testing.assert_allclose(Eh[k], Eo[k], rtol=1e-9, atol=1e-10, err_msg=k)
    gh, go = I.gains(ph), I.gains(po)
    np.testing.assert_allclose(gh["K"], go["K"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gh["d"], go["d"], rtol=1e-7, atol=1e-9)
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=70, **kw), hip, oracle)
    assert_solve_parity(T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve(), ph, po)
    def di3(lib):
        model = T.DoubleIntegrator(1.3, 3)
        n, m = model.dims()
        xf = np.concatenate([np.arange(1, 4, dtype=float), np.zeros(3)])
        obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 10.0 * np.ones(n), xf, 16)
        cons = T.ConstraintList(n, m, 16)
        T.add_constraint(cons, T.BoundConstraint(n, m, u_min=-2.0, u_max=2.0), range(1, 16))
        T.add_constraint(cons, T.GoalConstraint(xf), 16)
        p = T.Problem(model, obj, np.zeros(n), 2.0, xf=xf, constraints=cons, batch=5, lib=lib,
                      options=T.SolverOptions(lib=lib, constraint_tolerance=1e-5))
        p.set_initial_state(np.linspace(-0.5, 0.5, 5)[:, None] * np.ones((5, n)))
        return p
    ph, po = di3(hip), di3(oracle)
    assert_solve_parity(T.ALSolver(ph).solve(), T.ALSolver(po).solve(), ph, po)
    monkeypatch.setenv("TRAJOPT_FULL_COST_BLOCKS", "1")
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=40, constrained=True, **kw), hip, oracle)
    assert_solve_parity(T.ALSolver(ph).solve(), T.ALSolver(po).solve(), ph, po)


@pytest.mark.parametrize("depth", [1, 7, 33])
def test_line_search_depth_option(depth, hip, oracle):
    """iterations_linesearch other than the default 20 (fewer than one round, more than the candidate slots)."""
    def build(lib):
        o = T.SolverOptions(lib=lib, iterations_linesearch=depth, iterations=60)
        return configs.cartpole_problem(batch=48, lib=lib, options=o)
    ph, po = build(hip), build(oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)


def test_cost_kind_replaced_after_creation(hip, oracle):
    """set_cost switching a diagonal cost to a dense QuadraticCost must re-select the kernel variants (the diagonal-only
    expansion / forward kernels compile the dense branches out)."""
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=16, N=31, tf=1.5, **kw), hip, oracle)
    rng = np.random.default_rng(5)
    n, m = ph.n, ph.m
    A = rng.standard_normal((n, n)); Q = A @ A.T + np.eye(n)
    R = np.array([[0.3]]); H = 0.05 * rng.standard_normal((m, n))
    dense = T.QuadraticCost(Q, R, H=H, q=rng.standard_normal(n) * 0.1, r=np.array([0.02]), c=0.5)
    import ctypes as C
    for p in (ph, po):
        d = dense._desc()
        p._call("set_cost", 0, C.byref(d))  # cost 0 = the stage cost of Objective(stage, terminal, N)
    perturb_controls((ph, po), 0.05)
    T.rollout(ph); T.rollout(po)
    np.testing.assert_allclose(T.cost(ph), T.cost(po), rtol=1e-12)
    I.expand(ph); I.expand(po)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for key in Eo:
        np.testing.assert_allclose(Eh[key], Eo[key], rtol=1e-9, atol=1e-10, err_msg=key)
    sh, so = T.iLQRSolver(ph, iterations=30).solve(), T.iLQRSolver(po, iterations=30).solve()
    assert_solve_parity(sh, so, ph, po)


def test_tracking_mpc_resolves(hip, oracle):
    """MPC-style tracking: TrackingObjective + update_trajectory! between solves (src/objective.jl:185-212)."""
    model = T.Cartpole(); n, m = model.dims(); N = 31
    t = np.linspace(0, 1, 60)
    Xref = np.stack([0.3 * np.sin(2 * t), 0.2 * t, 0.6 * np.cos(2 * t), 0.2 + 0 * t]); Uref = 0.1 * np.cos(3 * t)[None, :-1]
    def build(lib):
        obj = T.TrackingObjective(np.array([5.0, 5.0, 0.1, 0.1]), np.array([0.05]), Xref[:, :N], Uref[:, :N], Qf=np.full(n, 20.0))
        p = T.Problem(model, obj, np.zeros(n), 1.5, batch=5, lib=lib)
        p.set_initial_state(np.tile(Xref[:, 0], (5, 1)) + 0.5 * np.arange(5)[:, None] * np.array([1.0, 1.0, 0.0, 0.0]))
        T.initial_controls(p, np.array([0.01]))
        return p
    ph, po = build(hip), build(oracle)
    for start in (1, 9, 20):
        for p in (ph, po):
            T.update_trajectory(p, Xref, Uref, start=start)
        sh, so = T.iLQRSolver(ph, iterations=40).solve(), T.iLQRSolver(po, iterations=40).solve()
        assert_solve_parity(sh, so, ph, po)


def test_error_quadratic_cost_on_gpu(hip, oracle):
    """ErrorQuadratic (src/lie_costs.jl:178-241): value, error-state expansion (gradient in dual numbers on the GPU vs the
    oracle's closed-form Hessian) and a full iLQR solve."""
    def build(lib):
        model = T.Quadrotor(); n, m = model.dims(); N = 41
        th = math.radians(60.0) / 2
        xf = np.zeros(n); xf[:3] = [0.8, -0.5, 0.6]; xf[3:7] = [math.cos(th), 0.0, math.sin(th), 0.0]
        Q = np.r_[np.ones(3), 2 * np.ones(3), 0.1 * np.ones(6)]
        R = np.full(m, 1e-2); u0 = model.hover_control()
        obj = T.Objective(T.ErrorQuadratic(model, Q, R, xf, u0), T.ErrorQuadratic(model, 100 * Q, R, xf, u0, terminal=True), N)
        x0 = np.zeros(n); x0[3] = 1
        p = T.Problem(model, obj, x0, 2.0, xf=xf, batch=12, lib=lib)
        p.set_initial_state(configs.quadrotor_x0(12))
        T.initial_controls(p, u0)
        return p
    ph, po = build(hip), build(oracle)
    perturb_controls((ph, po), 0.05)
    T.rollout(ph); T.rollout(po)
    np.testing.assert_allclose(T.stage_costs(ph), T.stage_costs(po), rtol=1e-12, atol=1e-14)
    gh, Hh = I.cost_gradient_hessian(ph); go, Ho = I.cost_gradient_hessian(po)
    np.testing.assert_allclose(gh, go, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(Hh, Ho, rtol=1e-9, atol=1e-9 * np.abs(Ho).max())
    I.expand(ph); I.expand(po)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for key in Eo:
        np.testing.assert_allclose(Eh[key], Eo[key], rtol=1e-9, atol=1e-10, err_msg=key)
    # the first iterations agree to 1e-6 with identical integer outputs; run to convergence the iteration paths of this
    # (non-convex, "not recommended" src/lie_costs.jl:210-212) cost separate chaotically like the AL tails,
    # so the converged solves are compared by outcome
    ph, po = build(hip), build(oracle)
    sh, so = T.iLQRSolver(ph, iterations=10).solve(), T.iLQRSolver(po, iterations=10).solve()
    assert_solve_parity(sh, so, ph, po)
    ph, po = build(hip), build(oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED) and np.all(so.stats["status"] == T.capi.SOLVE_SUCCEEDED)
    np.testing.assert_allclose(sh.stats["cost"], so.stats["cost"], rtol=1e-3)


def _random_config(seed):
    """A random problem from the supported space: model, horizon, batch, integrator, dt pattern, cost kinds, a random
    subset of constraints, a few solver options."""
    r = np.random.default_rng(seed)
    kind = r.choice(["di1", "di2", "di3", "cartpole", "quadrotor"])
    model = {"di1": T.DoubleIntegrator(1.0, 1), "di2": T.DoubleIntegrator(1.3, 2), "di3": T.DoubleIntegrator(0.7, 3),
             "cartpole": T.Cartpole(), "quadrotor": T.Quadrotor()}[kind]
    n, m = model.dims()
    N = int(r.integers(3, 34)); B = int(r.integers(1, 75)); tf = float(r.uniform(0.4, 2.0))
    integ = [T.RK4, T.RK3, T.Euler][int(r.integers(0, 3))]
    quad = kind == "quadrotor"
    xf = r.uniform(-0.5, 0.5, n)
    if quad:
        xf[3:7] = r.standard_normal(4); xf[3:7] /= np.linalg.norm(xf[3:7])
    u0 = model.hover_control() if quad else np.zeros(m)
    Qd, Rd = r.uniform(0.1, 2.0, n), r.uniform(0.05, 0.5, m)
    style = int(r.integers(0, 3))
    if quad and style == 0:
        stage, term = T.QuatLQRCost(Qd, Rd, xf, u0, w=float(r.uniform(0.2, 2))), T.QuatLQRCost(20 * Qd, Rd, xf, u0, terminal=True)
    elif style == 1:
        A = 0.1 * r.standard_normal((n, n)); Qm = np.diag(Qd) + A @ A.T
        Hm = 0.02 * r.standard_normal((m, n))
        stage = T.QuadraticCost(Qm, np.diag(Rd), Hm, -Qm @ xf, -Rd * u0, 0.1)
        term = T.LQRCost(20 * Qd, Rd, xf, u0, terminal=True)
    else:
        stage, term = T.LQRCost(Qd, Rd, xf, u0), T.LQRCost(20 * Qd, Rd, xf, u0, terminal=True)
    obj = T.Objective(stage, term, N)
    cons = T.ConstraintList(n, m, N)
    npos = 3 if quad else {"di1": 1, "di2": 2, "di3": 3, "cartpole": 1}[kind]
    with_cons = r.random() < 0.7
    if with_cons and r.random() < 0.5:
        T.add_constraint(cons, T.GoalConstraint(xf, list(range(1, npos + 1))), N)
    if not with_cons:
        pass
    elif r.random() < 0.5 and N > 2:
        T.add_constraint(cons, T.BoundConstraint(n, m, u_min=u0 - 3.0, u_max=u0 + 3.0), range(1, N))
    if with_cons and r.random() < 0.4 and N > 2:
        T.add_constraint(cons, T.NormConstraint(n, m, float(np.linalg.norm(u0) + 4.0), T.SecondOrderCone(), "control"), range(1, N))
    if with_cons and r.random() < 0.3 and n >= 2 and N > 3:
        T.add_constraint(cons, T.CircleConstraint(n, [0.9], [0.8], [0.2]), range(2, N))
    if with_cons and r.random() < 0.3 and N > 2:
        T.add_constraint(cons, T.LinearConstraint(n, m, r.standard_normal((1, 2)), np.array([4.0]), T.Inequality(), [1, n + 1]), range(1, N))
    dt = None
    if r.random() < 0.3:
        w = r.uniform(0.5, 1.5, N - 1); dt = tf * w / w.sum()
    opts = dict(cost_dt_scaling=int(r.random() < 0.3), iterations=int(r.integers(3, 25)), iterations_outer=int(r.integers(1, 4)),
                iterations_linesearch=int(r.integers(1, 24)), constraint_tolerance=1e-3)
    x0 = r.uniform(-0.3, 0.3, (B, n))
    if quad:
        x0[:, 3:7] = [1.0, 0, 0, 0]
    Uinit = np.tile(u0, (B, N - 1, 1)) + 0.05 * r.standard_normal((B, N - 1, m))

    def build(lib):
        p = T.Problem(model, obj, np.zeros(n), tf, xf=xf, constraints=cons, batch=B, integration=integ, dt=dt, lib=lib,
                      options=T.SolverOptions(lib=lib, **opts))
        p.set_initial_state(x0)
        T.initial_controls(p, Uinit)
        return p
    return build, len(cons) > 0, f"{kind} N={N} B={B} integ={integ} style={style} ncons={len(cons)} opts={opts}"


@pytest.mark.parametrize("seed", range(24))
def test_random_configurations(seed, hip, oracle):
    """Randomised drop-in check: any supported problem must give the oracle's phases and (short) solves."""
    build, constrained, desc = _random_config(1000 + seed)
    ph, po = build(hip), build(oracle)
    for p in (ph, po):
        T.rollout(p)
    np.testing.assert_allclose(T.states(ph), T.states(po), rtol=1e-10, atol=1e-12, err_msg=desc)
    np.testing.assert_allclose(T.cost(ph), T.cost(po), rtol=1e-11, err_msg=desc)
    for p in (ph, po):
        I.expand(p); I.backwardpass(p)
    Eh, Eo = I.cost_expansion(ph), I.cost_expansion(po)
    for key in Eo:
        np.testing.assert_allclose(Eh[key], Eo[key], rtol=1e-8, atol=1e-9 * (1 + np.abs(Eo[key]).max()), err_msg=desc + " " + key)
    gh, go = I.gains(ph), I.gains(po)
    np.testing.assert_array_equal(gh["rho"], go["rho"], err_msg=desc)
    np.testing.assert_allclose(gh["K"], go["K"], rtol=1e-6, atol=1e-8 * (1 + np.abs(go["K"]).max()), err_msg=desc)
    solver = T.ALSolver if constrained else T.iLQRSolver
    sh, so = solver(ph).solve(), solver(po).solve()
    for k in ("iterations", "iterations_outer", "status"):
        np.testing.assert_array_equal(sh.stats[k], so.stats[k], err_msg=desc + " " + k)
    # converged trajectories: the north-star tolerance; solves cut off by an iteration limit (or driven to the
    # regularisation limit) stop on an ill-conditioned iterate, where rounding differences are amplified: 1e-4
    done = so.stats["status"] == T.capi.SOLVE_SUCCEEDED
    np.testing.assert_allclose(sh.stats["cost"][done], so.stats["cost"][done], rtol=1e-6, err_msg=desc)
    np.testing.assert_allclose(sh.stats["cost"][~done], so.stats["cost"][~done], rtol=1e-4, err_msg=desc)
    Xh, Xo, Uh, Uo = T.states(ph), T.states(po), T.controls(ph), T.controls(po)
    tol = np.where(done, 1e-6, 1e-4)
    assert_trajectories_close(Xh, Xo, tol, desc + " X")
    assert_trajectories_close(Uh, Uo, tol, desc + " U")


def test_error_paths_on_device(hip):
    with pytest.raises(T.capi.ConeError):
        T.projection(T.SecondOrderCone(), np.array([np.nan, 1.0, 1.0]), lib=hip)
    p = configs.cartpole_problem(batch=2, N=5, tf=0.2, lib=hip)
    with pytest.raises(T.ArgumentError):
        p._call("set_cost", 7, None) if False else p._lib.call("set_cost", p._h, 7, T.capi.CostDesc())
    with pytest.raises(T.DimensionMismatch):
        T.initial_controls(p, np.zeros((3, 4, 1)))


def test_device_allgather_world1(hip):
    """The multi-GPU path of the C-ABI (to_comm_init_rank / to_allgather: RCCL all-gather of device-resident shards) with a
    world of one rank — the same code the N-rank bench runs — must return exactly what to_get_states / to_get_controls do;
    the device-to-device getters (to_get_*_device) likewise."""
    import ctypes as C
    import torch
    from trajectoryoptimization_jl_amd.distributed import TrajectoryGather
    p = configs.cartpole_problem(batch=70, N=41, tf=2.0, lib=hip)
    sv = T.iLQRSolver(p, iterations=15).solve()
    X, U = T.states(p), T.controls(p)
    g = TrajectoryGather(p, None, device=torch.device("cuda", 0))
    Xg, Ug = g()
    np.testing.assert_array_equal(Xg.cpu().numpy(), X)
    np.testing.assert_array_equal(Ug.cpu().numpy(), U)
    assert g.counts == [70] and g.total == 70      # to_comm_shards: what the RCCL communicator itself saw
    its, st, J = g.stats()                         # to_allgather_stats: the small gather of SURVEY §8e, through RCCL
    np.testing.assert_array_equal(its, sv.stats["iterations"])
    np.testing.assert_array_equal(st, sv.stats["status"])
    np.testing.assert_allclose(J, sv.stats["cost"], rtol=0, atol=0)
    with pytest.raises(T.ArgumentError):
        p._call("comm_init_rank", 1, 0, g._uid)   # already initialised
    g.close()
    xs = torch.empty((p.B, p.N, p.n), dtype=torch.float64, device="cuda")
    us = torch.empty((p.B, p.N - 1, p.m), dtype=torch.float64, device="cuda")
    p._call("get_states_device", C.c_void_p(xs.data_ptr()))
    p._call("get_controls_device", C.c_void_p(us.data_ptr()))
    np.testing.assert_array_equal(xs.cpu().numpy(), X)
    np.testing.assert_array_equal(us.cpu().numpy(), U)


def test_constraint_hessians_on_gpu(hip, oracle):
    """to_constraint_hessians (∇jacobian!, src/abstract_constraint.jl:255-280) for every kind with curvature, GPU vs oracle."""
    rng = np.random.default_rng(21)
    qf = rng.standard_normal(4)

    def build(lib):
        model = T.Quadrotor(); n, m = model.dims(); N = 9
        xf = np.zeros(n); xf[3] = 1
        obj = T.LQRObjective(np.ones(n), np.ones(m), np.ones(n), xf, N)
        cons = T.ConstraintList(n, m, N)
        T.add_constraint(cons, T.NormConstraint(n, m, 1.5, T.Inequality(), [8, 9, 10, 14]), range(1, N))
        T.add_constraint(cons, T.CircleConstraint(n, [0.25, -0.5], [0.1, 0.3], [0.05, 0.2]), range(1, N + 1))
        T.add_constraint(cons, T.SphereConstraint(n, [0.4], [0.4], [0.2], [0.05]), range(2, N + 1))
        T.add_constraint(cons, T.CollisionConstraint(n, [1, 2, 3], [8, 9, 10], 0.02), range(1, N + 1))
        T.add_constraint(cons, T.QuatVecEq(n, m, qf), range(1, N + 1))
        T.add_constraint(cons, T.GoalConstraint(xf), N)
        x0 = np.zeros(n); x0[3] = 1
        p = T.Problem(model, obj, x0, 1.0, xf=xf, constraints=cons, batch=70, lib=lib)
        p.set_initial_state(configs.quadrotor_x0(70))
        T.initial_controls(p, model.hover_control() + 0.3 * np.random.default_rng(3).standard_normal((70, N - 1, m)))
        T.rollout(p)
        return p
    ph, po = build(hip), build(oracle)
    for i, con in enumerate(ph.constraints):
        nk = ph.constraints.inds[i][1] - ph.constraints.inds[i][0] + 1
        lam = rng.standard_normal((ph.B, nk, con.p))
        w = T.constraint_jacobians(po, i).shape[3]
        H0 = rng.standard_normal((ph.B, nk, w, w))
        Hh, Ho = T.constraint_hessians(ph, i, lam, H=H0), T.constraint_hessians(po, i, lam, H=H0)
        np.testing.assert_allclose(Hh, Ho, rtol=1e-12, atol=1e-13, err_msg=type(con).__name__)


def test_indexed_constraints_solve(hip, oracle):
    """IndexedConstraint / change_dimension (src/constraints.jl:820-936): constraints written for a 2-D double integrator's
    dimensions, moved onto the x-y slice of a 3-D one, through a full AL solve on the GPU vs the oracle."""
    def build(lib):
        model = T.DoubleIntegrator(1.0, 3); n, m, N = 6, 3, 21
        xf = np.array([1.0, 2.0, 0.5, 0, 0, 0])
        obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 20.0 * np.ones(n), xf, N)
        inner = T.ConstraintList(2, 2, N)     # written for (position_xy, force_xy)
        T.add_constraint(inner, T.ControlBound(2, 2, u_max=1.5, u_min=-1.5), range(1, N))
        T.add_constraint(inner, T.NormConstraint(2, 2, 1.8, T.SecondOrderCone(), "control"), range(1, N))
        T.add_constraint(inner, T.CircleConstraint(2, [0.5], [1.0], [0.25]), range(2, N))
        T.add_constraint(inner, T.GoalConstraint(xf[:2]), N)
        cons = T.change_dimension(inner, n, m, ix=(1, 2), iu=(1, 2))
        T.add_constraint(cons, T.GoalConstraint(xf, [3, 4, 5, 6]), N)
        p = T.Problem(model, obj, np.zeros(n), 5.0, xf=xf, constraints=cons, batch=9, lib=lib,
                      options=T.SolverOptions(lib=lib, constraint_tolerance=1e-5))
        p.set_initial_state(np.linspace(-0.3, 0.3, 9)[:, None] * np.array([1.0, -1.0, 0.5, 0, 0, 0]))
        T.initial_controls(p, np.array([0.1, 0.2, 0.05]))
        return p
    ph, po = build(hip), build(oracle)
    for p in (ph, po):
        T.rollout(p)
    for i in range(len(ph.constraints)):
        np.testing.assert_allclose(T.evaluate_constraints(ph, i), T.evaluate_constraints(po, i), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(T.constraint_jacobians(ph, i), T.constraint_jacobians(po, i), rtol=1e-12, atol=1e-13)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po, rtol=1e-5)
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED)


@pytest.mark.parametrize("width", [16, 4])
def test_two_wave_forward_pass(width, hip, oracle, monkeypatch):
    """k_forward2 (a roller wave and an accountant wave per workgroup, an LDS ring between them) against k_forward: the same
    expressions in the same order, both compiled with -ffp-contract=on — BIT-IDENTICAL (the solve loop switches between them per
    batch step; with hipcc's default contraction they differed by 1e-13 per pass).  Constrained Quadrotor batch through the phase
    API (several line-search rounds with the narrow shape), then full iLQR / AL solves (compaction, deep shape) against the
    one-wave kernel and the oracle."""
    monkeypatch.setenv("TRAJOPT_LS_DEEP", "0")
    monkeypatch.setenv("TRAJOPT_LS_CANDIDATES", str(width))
    probs = []
    for two in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_FWD2", two)
        o = T.SolverOptions(lib=hip, constraint_tolerance=1e-4)
        p = configs.quadrotor_problem(batch=24, N=101, tf=5.0, constrained=True, lib=hip, options=o)
        T.rollout(p)
        probs.append(p)
    later_rounds = 0
    for it in range(36):
        out = []
        for p in probs:
            if it % 15 == 14:
                I.dual_update(p)
            I.expand(p); I.backwardpass(p)
            ls, J = I.forwardpass(p)
            out.append((ls, J, T.states(p), T.controls(p)))
        (l0, J0, X0, U0), (l1, J1, X1, U1) = out
        np.testing.assert_array_equal(l0, l1, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(J1, J0, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(X1, X0, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(U1, U0, err_msg=f"iteration {it}")
        later_rounds += int((l0 >= width).sum())
    assert width == 16 or later_rounds > 20
    monkeypatch.delenv("TRAJOPT_LS_DEEP")
    monkeypatch.delenv("TRAJOPT_LS_CANDIDATES")
    sols = []
    for two in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_FWD2", two)
        p = configs.quadrotor_problem(batch=37, N=61, tf=1.5, lib=hip)
        s = T.iLQRSolver(p, iterations=40).solve()
        o = T.SolverOptions(lib=hip, constraint_tolerance=1e-4)
        pc = configs.quadrotor_problem(batch=24, N=101, tf=5.0, constrained=True, lib=hip, options=o)
        sc = T.ALSolver(pc).solve()
        sols.append((s.stats["iterations"], s.stats["status"], sc.stats["iterations"], sc.stats["status"],
                     s.stats["cost"], T.states(p), T.controls(p), sc.stats["cost"], T.states(pc), T.controls(pc)))
    for x0, x1 in zip(*sols):   # whole solves, every output: bit for bit
        np.testing.assert_array_equal(x0, x1)
    monkeypatch.setenv("TRAJOPT_FWD2", "1")
    ph, po = pair(lambda **kw: configs.quadrotor_problem(batch=37, N=61, tf=1.5, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph, iterations=40).solve(), T.iLQRSolver(po, iterations=40).solve()
    assert_solve_parity(sh, so, ph, po)


@pytest.mark.parametrize("two", ["0", "1"])
@pytest.mark.parametrize("width", [4, 8])
def test_line_search_repack(width, two, hip, monkeypatch):
    """The repacked last round of the line search (k_forward.h LsRound: the trajectories of a wave that are still searching after
    the rounds of the static map share all 64 lanes for the remaining step sizes) against rounds of the static map only
    (TRAJOPT_LS_REPACK=0): BIT-IDENTICAL accepted steps, costs and trajectories — through the phase API on a constrained
    Quadrotor batch with dual updates (deep searches, failed searches), one-wave and two-wave kernels, then whole AL solves."""
    monkeypatch.setenv("TRAJOPT_LS_DEEP", "0")
    monkeypatch.setenv("TRAJOPT_LS_CANDIDATES", str(width))
    monkeypatch.setenv("TRAJOPT_FWD2", two)
    probs = []
    for rp in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_LS_REPACK", rp)
        o = T.SolverOptions(lib=hip, constraint_tolerance=1e-4)
        p = configs.quadrotor_problem(batch=44, N=101, tf=5.0, constrained=True, lib=hip, options=o)
        T.rollout(p)
        probs.append(p)
    deep = 0
    for it in range(40):
        out = []
        for p in probs:
            if it % 12 == 11:
                I.dual_update(p)
            I.expand(p); I.backwardpass(p)
            ls, J = I.forwardpass(p)
            out.append((ls, J, T.states(p), T.controls(p)))
        (l0, J0, X0, U0), (l1, J1, X1, U1) = out
        np.testing.assert_array_equal(l0, l1, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(J1, J0, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(X1, X0, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(U1, U0, err_msg=f"iteration {it}")
        deep += int((l0 >= width).sum()) + int((l0 < 0).sum())
    assert deep > 20, "the searches never went past the first round"
    sols = []
    for rp in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_LS_REPACK", rp)
        o = T.SolverOptions(lib=hip, constraint_tolerance=1e-4)
        pc = configs.quadrotor_problem(batch=40, N=101, tf=5.0, constrained=True, lib=hip, options=o)
        sc = T.ALSolver(pc).solve()
        sols.append((sc.stats, T.states(pc), T.controls(pc)))
    for k in ("iterations", "status", "cost"):
        np.testing.assert_array_equal(sols[0][0][k], sols[1][0][k], err_msg=k)
    np.testing.assert_array_equal(sols[0][1], sols[1][1])
    np.testing.assert_array_equal(sols[0][2], sols[1][2])


def test_line_search_deeper_than_the_deep_shape(hip, oracle, monkeypatch):
    """The search depth raised AFTER the handle was created (the deep wave shape was sized for 20 step sizes; a solver object sets
    40): the rounds beyond the deep shape's first one repack into the second set of candidate blocks, which must cover the deep
    shape's wave count.  A strict acceptance window makes searches go that deep.  Equal with and without repacking; oracle parity."""
    kw = dict(iterations_linesearch=40, line_search_lower_bound=0.35, line_search_upper_bound=1.5, iterations=25)
    sols = []
    for rp in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_LS_REPACK", rp)
        p = configs.quadrotor_problem(batch=64, N=61, tf=1.5, lib=hip)
        s = T.iLQRSolver(p, **kw).solve()
        sols.append((s.stats, T.states(p), T.controls(p)))
    for k in ("iterations", "status", "cost"):
        np.testing.assert_array_equal(sols[0][0][k], sols[1][0][k], err_msg=k)
    np.testing.assert_array_equal(sols[0][1], sols[1][1])
    np.testing.assert_array_equal(sols[0][2], sols[1][2])
    po = configs.quadrotor_problem(batch=64, N=61, tf=1.5, lib=oracle)
    so = T.iLQRSolver(po, **kw).solve()
    np.testing.assert_array_equal(sols[1][0]["iterations"], so.stats["iterations"])
    np.testing.assert_allclose(sols[1][1], T.states(po), rtol=1e-6, atol=1e-8)


def _mrp_quadrotor(lib, constrained, batch, N=41, tf=2.0, integration=T.RK4, options=None):
    model = T.Quadrotor(rotation="mrp")
    n, m = model.dims()
    th = math.radians(70.0) / 2
    xf = model.build_state([1.0, 1.5, 0.5], [math.cos(th), 0.0, 0.0, math.sin(th)])
    Qe = np.r_[np.ones(3), 0.5 * np.ones(3), 0.1 * np.ones(6)]
    stage = T.ErrorQuadratic(model, Qe, np.full(m, 1e-2), xf, model.hover_control())
    term = T.ErrorQuadratic(model, 100 * Qe, np.full(m, 1e-2), xf, model.hover_control(), terminal=True)
    cons = T.ConstraintList(n, m, N)
    if constrained:
        T.add_constraint(cons, T.BoundConstraint(n, m, u_min=0.0, u_max=2.2), range(1, N))
        T.add_constraint(cons, T.GoalConstraint(xf, [1, 2, 3, 7, 8, 9, 10, 11, 12]), N)
    prob = T.Problem(model, T.Objective(stage, term, N), np.zeros(n), tf, xf=xf, constraints=cons, batch=batch, lib=lib,
                     integration=integration, options=options)
    rng = np.random.default_rng(11)
    x0 = np.zeros((batch, n)); x0[:, :3] = rng.uniform(-0.5, 0.5, (batch, 3)); x0[:, 3:6] = 0.1 * rng.standard_normal((batch, 3))
    prob.set_initial_state(x0)
    T.initial_controls(prob, model.hover_control())
    return prob


@pytest.mark.parametrize("att", ["quat", "mrp"])
def test_accept_by_rollout(att, hip, oracle, monkeypatch):
    """Batch steps whose forward pass fills the chip store only the candidates' controls and re-roll the accepted ones
    (k_accept_roll, TRAJOPT_ACCEPT_ROLL_MIN): the nominal states must be BIT-IDENTICAL to the stored-candidate path (same step
    function, -ffp-contract=on) — iLQR and AL solves, states, controls, costs and iteration counts compared for equality; then
    against the oracle."""
    sols = []
    for waves in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_MIN", waves)
        if att == "quat":
            p = configs.quadrotor_problem(batch=200, N=61, tf=1.5, lib=hip)
            o = T.SolverOptions(lib=hip, constraint_tolerance=1e-4)
            pc = configs.quadrotor_problem(batch=72, N=101, tf=5.0, constrained=True, lib=hip, options=o)
        else:
            p, pc = _mrp_quadrotor(hip, False, 100), _mrp_quadrotor(hip, True, 40)
        s = T.iLQRSolver(p, iterations=60).solve()
        sc = T.ALSolver(pc).solve()
        sols.append((s.stats, T.states(p), T.controls(p), sc.stats, T.states(pc), T.controls(pc)))
    a, b = sols
    for k in ("iterations", "status", "cost"):
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
        np.testing.assert_array_equal(a[3][k], b[3][k], err_msg="AL " + k)
    for i in (1, 2, 4, 5):
        np.testing.assert_array_equal(a[i], b[i])
    assert a[0]["iterations"].max() > 3 and (a[3]["iterations"] > 10).any()
    if att == "quat":
        po = configs.quadrotor_problem(batch=200, N=61, tf=1.5, lib=oracle)
        so = T.iLQRSolver(po, iterations=60).solve()
        np.testing.assert_array_equal(b[0]["iterations"], so.stats["iterations"])
        np.testing.assert_allclose(b[1], T.states(po), rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("case", ["cartpole", "cartpole_lane", "cartpole_al", "quickstart", "hybrid", "vector"])
def test_accept_by_rollout_small_models(case, hip, monkeypatch):
    """The same for the small (write-through) models, whose large batches live on it by default (from 32 768 active trajectories on):
    candidate controls only, k_accept_roll on this step's active list, the next expansion reads the nominal instead of gathering the
    accepted candidate.  Whole solves must be BIT-IDENTICAL with the path forced on (every batch step) and off — on the scan /
    cooperative path, on the fused lane path with compaction (ragged batch, part of it converged), AL solves, the hybrid model
    vector and the general one."""
    monkeypatch.setenv("TRAJOPT_FWD2", "0")   # (two-wave workgroups always store whole candidates)
    if case == "cartpole_lane":
        monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")
    sols = []
    for roll in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_MIN", roll)
        if case == "cartpole":
            p = configs.cartpole_problem(batch=96, lib=hip); s = T.iLQRSolver(p).solve()
        elif case == "cartpole_lane":
            p = configs.cartpole_problem(batch=5000, N=41, tf=2.0, lib=hip); s = T.iLQRSolver(p, iterations=40).solve()
        elif case == "cartpole_al":
            p = configs.cartpole_problem(batch=70, constrained=True, lib=hip); s = T.ALSolver(p).solve()
        elif case == "quickstart":
            p = configs.quickstart_problem(batch=3, lib=hip); s = T.ALSolver(p).solve()
        elif case == "hybrid":
            from test_hybrid_dims import hybrid_problem
            (p, _, _, _) = hybrid_problem(hip, batch=200); s = T.iLQRSolver(p).solve()
        else:
            from test_model_vector import build, cartpole_mix
            (p, _, _) = build(cartpole_mix(), hip, batch=70); s = T.iLQRSolver(p).solve()
        info = (ctypes.c_int32 * 8)()
        p._call("solver_path", info)
        assert info[6] == (1 if roll == "1" else 0)
        sols.append(({k: np.array(v).copy() for k, v in s.stats.items()}, T.states(p), T.controls(p), s.batch_steps))
    (s0, X0, U0, n0), (s1, X1, U1, n1) = sols
    assert n0 == n1 and s0["iterations"].max() >= 2
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    np.testing.assert_array_equal(X0, X1)
    np.testing.assert_array_equal(U0, U1)


@pytest.mark.parametrize("goals,at", [(False, "0.7"), (True, "0.5"), (False, "0.3")])
def test_repacked_working_set(goals, at, hip, monkeypatch):
    """Once the active count of a large batch has halved, the solve loop moves the state of the trajectories still being solved into a
    dense working set and goes on there (k_generic.h k_repack_*), again and again as the batch drains; finished trajectories go back
    to their home position.  Which position holds a trajectory changes nothing in its arithmetic: every output must be BIT-IDENTICAL
    to the solve that never moves anything (TRAJOPT_REPACK=0) — 70 000 Cartpole trajectories, moves allowed down to 2 048 (so that
    several happen, across the change of compaction kernels at 16 384 and of the accept path at 32 768), with and without one goal per
    trajectory (the per-trajectory cost terms travel with the state)."""
    out = []
    monkeypatch.setenv("TRAJOPT_REPACK_AT", at)     # the fraction of the working set that has to be left for a move
    for rp in ("0", "2048"):
        monkeypatch.setenv("TRAJOPT_REPACK", rp)
        p = configs.cartpole_problem(batch=70000, N=41, tf=2.0, lib=hip)
        if goals:
            Xf = np.tile(p.xf, (p.B, 1)); Xf[:, 0] = np.random.default_rng(1).uniform(-1, 1, p.B)
            T.set_goal_state(p, Xf)
        s = T.iLQRSolver(p, iterations=80).solve()
        out.append(({k: np.array(v).copy() for k, v in s.stats.items()}, T.states(p), T.controls(p), s.batch_steps, T.cost(p)))
        s2 = T.iLQRSolver(p, iterations=80).solve()       # a second solve on the same handle starts from the home arrays again
        assert s2.batch_steps >= 1
    (s0, X0, U0, n0, J0), (s1, X1, U1, n1, J1) = out
    assert n0 == n1 and 0.02 < np.mean(s0["status"] == T.capi.SOLVE_SUCCEEDED) and len(set(s0["iterations"])) > 10
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    np.testing.assert_array_equal(X0, X1); np.testing.assert_array_equal(U0, U1); np.testing.assert_array_equal(J0, J1)


def test_two_launch_line_search(hip, monkeypatch):
    """Large dense batches of the small models run the line search in two launches (common.h ls_phase): one round for every active
    trajectory, a compaction of the trajectories that accepted nothing yet, the rest of the search for those only.  Same candidates,
    same first accepted step size: whole solves must be BIT-IDENTICAL to the one-launch search, whatever the widths of the two launches —
    33 000 Cartpole trajectories (ragged last tile), the re-roll path forced on for every batch step so that the two-launch search
    serves the thinning batch as well, 40 iterations (part of the batch converged, searches of every depth)."""
    monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_MIN", "1")
    monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_FRAC", "0")
    out = []
    for two in ("0", "1,2", "2,2", "1,4", "3,1"):
        monkeypatch.setenv("TRAJOPT_LS_TWO", two)
        p = configs.cartpole_problem(batch=33000, N=41, tf=2.0, lib=hip)
        s = T.iLQRSolver(p, iterations=40).solve()
        out.append(({k: np.array(v).copy() for k, v in s.stats.items()}, T.states(p), T.controls(p), s.batch_steps))
    ref = out[0]
    assert len(set(ref[0]["iterations"])) > 5
    for st, X, U, n in out[1:]:
        assert n == ref[3]
        for k in st:
            np.testing.assert_array_equal(st[k], ref[0][k], err_msg=k)
        np.testing.assert_array_equal(X, ref[1])
        np.testing.assert_array_equal(U, ref[2])


@pytest.mark.parametrize("two", ["0", "1"])
def test_two_wave_forward_pass_small_models(two, hip, oracle, monkeypatch):
    """The small models' forward pass (gains row in registers, accepted steps written through by the next expansion) with one
    wave per candidate group (TRAJOPT_FWD2=0) and as roller + accountant workgroups (=1; the default picks per batch step):
    both against the oracle — Cartpole iLQR and AL (C2 shapes), a line search that goes into later rounds, and the quickstart
    problem (2-D double integrator, bounds, obstacles, goal)."""
    monkeypatch.setenv("TRAJOPT_FWD2", two)
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=96, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=40, constrained=True, **kw), hip, oracle)
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    monkeypatch.setenv("TRAJOPT_LS_CANDIDATES", "1")
    ph, po = pair(lambda **kw: configs.cartpole_problem(batch=33, **kw), hip, oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    monkeypatch.delenv("TRAJOPT_LS_CANDIDATES")
    ph, po = pair(BUILDERS["quickstart"], hip, oracle)   # 2-D double integrator, bounds + circle obstacles + goal
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)


@pytest.mark.parametrize("mix", ["linear", "cartpole"])
def test_general_model_vector_on_gpu(mix, hip, oracle):
    """Problem(models::Vector, ...) in general (TO_MODEL_VECTOR; src/dynamics.jl:15-31): double integrators of three sizes, Cartpoles
    and linear jump maps chained, through the per-step table on the device.  Every phase against the oracle (whose solve is pinned
    against a Riccati recursion at the true per-knot dimensions in tests/test_model_vector.py), then iLQR, AL and ALTRO solves."""
    from test_model_vector import build, cartpole_mix, linear_mix
    models = linear_mix() if mix == "linear" else cartpole_mix()
    (ph, _, _), (po, _, _) = build(models, hip, batch=70), build(models, oracle, batch=70)
    assert ph.knot_dims() == po.knot_dims() == (ph.nx, ph.nu)
    rng = np.random.default_rng(4)
    U = np.zeros((70, ph.N - 1, ph.m))
    for k, mk in enumerate(ph.nu[:-1]):
        U[:, k, :mk] = rng.uniform(-1, 1, (70, mk))
    for p in (ph, po):
        T.initial_controls(p, U); T.rollout(p)
    np.testing.assert_allclose(T.states(ph), T.states(po), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(T.cost(ph), T.cost(po), rtol=1e-12)
    for p in (ph, po):
        I.expand(p); I.backwardpass(p)
    (Ah, Bh), (Ao, Bo) = I.dynamics_jacobians(ph), I.dynamics_jacobians(po)
    np.testing.assert_allclose(Ah, Ao, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(Bh, Bo, rtol=1e-10, atol=1e-12)
    gh, go = I.gains(ph), I.gains(po)
    np.testing.assert_allclose(gh["K"], go["K"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gh["d"], go["d"], rtol=1e-7, atol=1e-9)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    X = T.states(ph)
    for k in range(ph.N):
        np.testing.assert_array_equal(X[:, k, ph.nx[k]:], 0.0)      # the padding stays exactly zero
    (pc, _, _), (oc, _, _) = build(models, hip, batch=37, constrained=True), build(models, oracle, batch=37, constrained=True)
    assert_solve_parity(T.ALSolver(pc).solve(), T.ALSolver(oc).solve(), pc, oc)
    (pc, _, _), (oc, _, _) = build(models, hip, batch=37, constrained=True), build(models, oracle, batch=37, constrained=True)
    sh, so = T.ALTROSolver(pc).solve(), T.ALTROSolver(oc).solve()
    for k in ("iterations", "iterations_outer", "iterations_pn", "status"):
        np.testing.assert_array_equal(sh.stats[k], so.stats[k], err_msg=k)
    assert_trajectories_close(T.states(pc), T.states(oc), 1e-6, "X")
    assert_trajectories_close(T.controls(pc), T.controls(oc), 1e-6, "U")
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED) and sh.stats["c_max"].max() <= 1e-6


@pytest.mark.parametrize("path", ["default", "lane", "split"])
def test_hybrid_model_vector_on_gpu(path, hip, oracle, monkeypatch):
    """SURVEY §8(f)4, test/hybrid_dynamics_model.jl: the model vector 2-D double integrator x 5 -> jump map -> 1-D double
    integrator x 4 (TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, states / controls zero-padded at (4, 2)) on every small-model kernel path:
    fused cooperative (default), one lane per trajectory with chunk-mode duals (fused lane), and the split expansion + backward
    kernels.  Each phase against the oracle (whose solve is pinned against a Riccati recursion at the true per-knot dimensions in
    tests/test_hybrid_dims.py), then iLQR and AL solves; the padding must stay exactly zero."""
    from test_hybrid_dims import hybrid_problem
    if path == "lane":
        monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")
    elif path == "split":
        monkeypatch.setenv("TRAJOPT_FUSED_COOP", "0")
    batch = 70
    (ph, costs, x0, hyb), (po, _, _, _) = hybrid_problem(hip, batch=batch), hybrid_problem(oracle, batch=batch)
    assert ph.knot_dims() == po.knot_dims() == (ph.nx, ph.nu)
    rng = np.random.default_rng(2)
    x0b = np.zeros((batch, 4)); x0b[:] = x0; x0b += 0.3 * rng.standard_normal((batch, 4))
    U0 = 0.2 * rng.standard_normal((batch, ph.N - 1, 2)); U0[:, 6:, 1] = 0.0   # the padded control of the 1-D steps is zero by contract
    for p in (ph, po):
        p.set_initial_state(x0b); T.initial_controls(p, U0); T.rollout(p)
    np.testing.assert_allclose(T.states(ph), T.states(po), rtol=1e-13, atol=1e-14)
    np.testing.assert_array_equal(T.states(ph)[:, 6:, 2:], 0.0)
    np.testing.assert_allclose(T.cost(ph), T.cost(po), rtol=1e-13)
    np.testing.assert_allclose(I.discrete_jacobian(ph), I.discrete_jacobian(po), rtol=1e-12, atol=1e-14)
    for p in (ph, po):
        I.expand(p); I.backwardpass(p)
    (Ah, Bh), (Ao, Bo) = I.dynamics_jacobians(ph), I.dynamics_jacobians(po)
    np.testing.assert_allclose(Ah, Ao, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(Bh, Bo, rtol=1e-12, atol=1e-14)
    kh, ko = I.gains(ph), I.gains(po)
    np.testing.assert_allclose(kh["K"], ko["K"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(kh["d"], ko["d"], rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(kh["K"][:, 6:, 1, :], 0.0)    # no feedback onto a padded control
    np.testing.assert_array_equal(kh["d"][:, 6:, 1], 0.0)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED)
    np.testing.assert_array_equal(T.states(ph)[:, 6:, 2:], 0.0)
    np.testing.assert_array_equal(T.controls(ph)[:, 6:, 1], 0.0)
    (ph, _, _, _), (po, _, _, _) = hybrid_problem(hip, batch=batch, constrained=True), hybrid_problem(oracle, batch=batch, constrained=True)
    for p in (ph, po):
        p.set_initial_state(x0b)
    assert T.num_constraints(ph) == [4, 4, 4, 4, 4, 0, 3, 3, 3, 3, 2]
    sh, so = T.ALSolver(ph).solve(), T.ALSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    done = sh.stats["status"] == T.capi.SOLVE_SUCCEEDED   # (a few of the perturbed starts run into the iteration limit, on the oracle alike)
    assert done.mean() > 0.9 and np.all(sh.stats["c_max"][done] < 1e-6)
    np.testing.assert_array_equal(T.controls(ph)[:, 6:, 1], 0.0)


def test_hybrid_model_vector_large_batch_on_gpu(hip, oracle, monkeypatch):
    """The same model vector on the throughput path — fused lane kernel + active-list compaction (the default from ~20 000
    unconstrained trajectories on; forced here at 12 325): a sample of trajectories against the oracle."""
    from test_hybrid_dims import hybrid_problem
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")
    batch = 12288 + 37
    (ph, _, x0, _) = hybrid_problem(hip, batch=batch)
    rng = np.random.default_rng(4)
    x0b = np.zeros((batch, 4)); x0b[:] = x0; x0b += 0.3 * rng.standard_normal((batch, 4))
    ph.set_initial_state(x0b)
    sh = T.iLQRSolver(ph).solve()
    assert np.all(sh.stats["status"] == T.capi.SOLVE_SUCCEEDED)
    idx = rng.choice(batch, 64, replace=False)
    (po, _, _, _) = hybrid_problem(oracle, batch=64)
    po.set_initial_state(x0b[idx])
    so = T.iLQRSolver(po).solve()
    np.testing.assert_array_equal(sh.stats["iterations"][idx], so.stats["iterations"])
    np.testing.assert_allclose(sh.stats["cost"][idx], so.stats["cost"], rtol=1e-9)
    np.testing.assert_allclose(T.states(ph)[idx], T.states(po), rtol=1e-7, atol=1e-9)


def test_scan_backward_pass(hip, oracle, monkeypatch):
    """k_expand_backward_scan (k_scan.h): the Riccati recursion as an associative scan over the horizon — one wave per trajectory,
    two knots per lane — against the oracle's sequential recursion.  Gains and expected improvement through the phase API
    (TRAJOPT_SCAN=2 routes to_backward through the solve loop's kernel), on the initial guess and on iterates of the solve; a
    trajectory with pending regularisation (rho > 0: no Riccati recursion, no scan) takes the sequential pass inside the same
    kernel and must match the oracle's sequential pass to the last digits; then full solves with the scan on (default) and off:
    identical integers, results within the band."""
    monkeypatch.setenv("TRAJOPT_SCAN", "2")
    for name, batch in (("cartpole", 70), ("di", 5)):
        def build(lib):
            if name == "cartpole":
                return configs.cartpole_problem(batch=batch, lib=lib)
            model = T.DoubleIntegrator(1.0, 2)
            N = 21
            obj = T.LQRObjective(np.ones(4), 0.1 * np.ones(2), 10 * np.ones(4), np.array([1.0, 2.0, 0, 0]), N)
            p = T.Problem(model, obj, np.zeros(4), 3.0, batch=batch, lib=lib)
            T.initial_controls(p, np.array([0.1, 0.0]))
            return p
        ph, po = build(hip), build(oracle)
        for it in range(6):
            for p in (ph, po):
                if it == 0:
                    T.rollout(p)
                I.expand(p); I.backwardpass(p)
            kh, ko = I.gains(ph), I.gains(po)
            np.testing.assert_array_equal(kh["rho"], ko["rho"])
            # iteration 0: the same inputs to the last bit — the scan's own rounding (2e-15 of the largest gain in the numpy
            # prototype); later iterates have drifted apart by what the solve amplifies (1e8 on this problem: DESIGN.md §2)
            tolK, told = (1e-13, 1e-12) if it == 0 else (1e-9, 1e-8)
            scale = np.abs(ko["K"]).max(axis=(1, 2, 3), keepdims=True)
            assert np.max(np.abs(kh["K"] - ko["K"]) / scale) < tolK, f"{name} iteration {it}"
            dscale = np.maximum(np.abs(ko["d"]).max(axis=(1, 2), keepdims=True), 1e-6)   # (an exactly solved LQ problem leaves d = rounding noise)
            assert np.max(np.abs(kh["d"] - ko["d"]) / dscale) < told, f"{name} iteration {it}"
            np.testing.assert_allclose(kh["dV"], ko["dV"], rtol=1e-12 if it == 0 else 1e-8, atol=1e-18)
            for p in (ph, po):
                I.forwardpass(p)
    # regularisation pending from the start (bp_reg_initial > 0): the in-kernel sequential pass, phase API and full solve
    def build_reg(lib):
        return configs.cartpole_problem(batch=33, lib=lib, options=T.SolverOptions(lib=lib, bp_reg_initial=5.0))
    ph, po = build_reg(hip), build_reg(oracle)
    for p in (ph, po):
        T.rollout(p); I.expand(p); I.backwardpass(p)
    kh, ko = I.gains(ph), I.gains(po)
    np.testing.assert_allclose(kh["K"], ko["K"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(kh["d"], ko["d"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(kh["dV"], ko["dV"], rtol=1e-12)
    np.testing.assert_array_equal(kh["rho"], ko["rho"])
    ph, po = build_reg(hip), build_reg(oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
    # full solves: scan on / off / oracle
    sols = {}
    for scan in ("1", "0"):
        monkeypatch.setenv("TRAJOPT_SCAN", scan)
        p = configs.cartpole_problem(batch=200, lib=hip)
        s = T.iLQRSolver(p).solve()
        sols[scan] = (s, p)
    po = configs.cartpole_problem(batch=200, lib=oracle)
    so = T.iLQRSolver(po).solve()
    for scan in ("1", "0"):
        s, p = sols[scan]
        assert_solve_parity(s, so, p, po)


@pytest.mark.parametrize("N", [2, 3, 4, 21, 64, 65, 126, 127])
def test_scan_backward_pass_horizons(N, hip, oracle, monkeypatch):
    """The scan kernel's block / lane bookkeeping over horizons from the degenerate (N = 2: one stage knot and the terminal one in the
    same block) to the largest it takes (N = 126: 63 blocks; 127 falls back to the cooperative kernel), odd and even: gains on the
    initial guess and full solves against the oracle, for the 2-D double integrator (m = 2) and the Cartpole (m = 1)."""
    monkeypatch.setenv("TRAJOPT_SCAN", "2")

    def build_di(lib):
        model = T.DoubleIntegrator(1.0, 2)
        obj = T.LQRObjective(np.array([1.0, 2.0, 0.5, 0.3]), np.array([0.1, 0.2]), 10 * np.ones(4), np.array([1.0, 2.0, 0, 0]), N)
        p = T.Problem(model, obj, np.array([0.2, -0.1, 0.0, 0.3]), 0.1 * (N - 1), batch=9, lib=lib)
        T.initial_controls(p, np.array([0.1, -0.05]))
        return p

    def build_cp(lib):
        return configs.cartpole_problem(batch=9, N=N, tf=0.05 * (N - 1), lib=lib)

    for build in (build_di, build_cp):
        ph, po = build(hip), build(oracle)
        for p in (ph, po):
            T.rollout(p); I.expand(p); I.backwardpass(p)
        kh, ko = I.gains(ph), I.gains(po)
        scale = max(np.abs(ko["K"]).max(), 1e-30)
        assert np.abs(kh["K"] - ko["K"]).max() / scale < 1e-12
        assert np.abs(kh["d"] - ko["d"]).max() / max(np.abs(ko["d"]).max(), 1e-9) < 1e-11
        np.testing.assert_allclose(kh["dV"], ko["dV"], rtol=1e-11, atol=1e-20)
        ph, po = build(hip), build(oracle)
        sh, so = T.iLQRSolver(ph, iterations=25).solve(), T.iLQRSolver(po, iterations=25).solve()
        assert_solve_parity(sh, so, ph, po, unconverged_rtol=1e-4)


@pytest.mark.parametrize("kind", ["cartpole", "cartpole_big", "quadrotor", "quadrotor_al"])
def test_state_and_control_limits_of_the_initial_rollout(kind, hip, oracle):
    """TO_STATE_LIMIT / TO_CONTROL_LIMIT (Altro's rollout! check, knot by knot: the state first, then the control): trajectories whose
    INITIAL rollout leaves the limits end with that status and no iteration, on every solver path — cooperative / scan (small batch),
    fused lane with compaction (large batch), MFMA with compaction (Quadrotor), AL — and the rest of the batch solves as if they were
    not there (integers bit-exact against the oracle)."""
    def mk(lib):
        if kind == "cartpole":
            return configs.cartpole_problem(batch=70, N=41, tf=2.0, lib=lib)
        if kind == "cartpole_big":
            return configs.cartpole_problem(batch=40000, N=21, tf=1.0, lib=lib)
        if kind == "quadrotor_al":  # (the C5 shape of test_al_solve_quadrotor_soc: tolerance 1e-4 keeps the AL solve out of its chaotic tail)
            return configs.quadrotor_problem(batch=24, N=101, tf=5.0, constrained=True, lib=lib, options=T.SolverOptions(lib=lib, constraint_tolerance=1e-4))
        return configs.quadrotor_problem(batch=48, N=41, tf=1.0, lib=lib)
    ph, po = mk(hip), mk(oracle)
    B, N, m = ph.B, ph.N, ph.m
    U = T.controls(ph).copy()
    bad_u, bad_x, bad_nan = [1, B // 2, B - 1], [3, B // 2 + 1], [5]
    cart = kind.startswith("cartpole")
    lim = dict(max_control_value=50.0, max_state_value=30.0 if cart else 2000.0)  # (2000: far from anything a line-search candidate of the healthy trajectories reaches — the limit test is a sharp threshold)
    for b in bad_u:
        U[b, 7, 0] = 60.0        # beyond max_control_value at knot 8; the state it produces stays inside
    for b in bad_x:
        U[b, :, 0] = 40.0        # legal, and drives a velocity through max_state_value within ten knots
    U[bad_nan[0], 2, m - 1] = float("nan")
    for p in (ph, po):
        T.initial_controls(p, U)
    Solver = T.ALSolver if kind == "quadrotor_al" else T.iLQRSolver
    kw = dict(iterations=12, **lim) if kind == "cartpole_big" else dict(lim)
    sh, so = Solver(ph, **kw).solve(), Solver(po, **kw).solve()
    for k in ("status", "iterations", "iterations_outer", "iterations_pn"):
        np.testing.assert_array_equal(sh.stats[k], so.stats[k], err_msg=k)
    st = sh.stats["status"]
    assert (st[bad_u] == T.capi.CONTROL_LIMIT).all() and (st[bad_x] == T.capi.STATE_LIMIT).all() and st[bad_nan[0]] == T.capi.STATE_LIMIT
    assert sh.stats["iterations"][bad_u + bad_x + bad_nan].max() == 0
    ok = np.ones(B, bool); ok[bad_u + bad_x + bad_nan] = False
    assert sh.stats["iterations"][ok].min() >= 1
    np.testing.assert_allclose(T.states(ph)[ok], T.states(po)[ok], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(T.controls(ph)[ok], T.controls(po)[ok], rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("integration", [T.RK4, T.RK3, T.Euler])
@pytest.mark.parametrize("constrained", [False, True])
def test_packed_quadrotor_expansion_is_bit_identical(integration, constrained, hip, monkeypatch):
    """The packed expansion of the quaternion rigid body (k_expand.h PACK: six trajectories x the ten differentiated columns per wave, the six
    constant columns of [A B] written once per handle, their cost entries delivered through a superposed direction) against the 4 x 16 kernel
    (TRAJOPT_EXPAND_PACK=0): every block the backward pass reads — A, B, the compact cost block, the gradients — and whole iLQR / ALTRO solves
    must be EQUAL, for every integrator (the constant column mirrors the dual numbers' roundings), with ragged batches (41 = 6 x 6 + 5) and
    after the constraint list was switched to the general variant and back (which overwrites the constant columns in between)."""
    out = []
    for pack in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_EXPAND_PACK", pack)
        p = configs.quadrotor_problem(batch=41, N=52, tf=2.0, constrained=constrained, goal_inds=configs.C5_GOAL_INDS, integration=integration, lib=hip)
        perturb_controls((p,), 0.05)
        T.rollout(p)
        if constrained:
            I.dual_update(p); I.dual_update(p)
            Xf = np.tile(p.xf, (p.B, 1)); Xf[:, 0] += 0.1
            T.set_goal_state(p, Xf)            # general variant (full cost block, 4 x 16 kernel) ...
            I.expand(p)
            T.set_goal_state(p, p.xf)          # ... and back to the compact block: the constant columns are restored
        I.expand(p)
        A, Bm = I.dynamics_jacobians(p)
        ce = I.cost_expansion(p)
        I.backwardpass(p)
        g = I.gains(p)
        s = (T.ALTROSolver(p, n_steps=configs.C5_PN_STEPS) if constrained else T.iLQRSolver(p, iterations=40)).solve()
        out.append((A, Bm, ce, g, {k: v.copy() for k, v in s.stats.items()}, T.states(p), T.controls(p)))
    (A0, B0, c0, g0, s0, X0, U0), (A1, B1, c1, g1, s1, X1, U1) = out
    np.testing.assert_array_equal(A0, A1); np.testing.assert_array_equal(B0, B1)
    assert np.all(A1[:, :, :3, :3] == np.eye(3)) and np.all(A1[:, :, 6:9, 6:9] == np.eye(3)) and np.all(A1[:, :, 3:, :3] == 0)
    for k in c0:
        np.testing.assert_array_equal(c0[k], c1[k], err_msg=k)
    for k in ("K", "d"):
        np.testing.assert_array_equal(g0[k], g1[k], err_msg=k)
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    np.testing.assert_array_equal(X0, X1); np.testing.assert_array_equal(U0, U1)
    assert s1["iterations"].min() >= 3


@pytest.mark.parametrize("rot", ["mrp", "rp"])
def test_packed_expansion_three_parameter_attitudes(rot, hip, oracle, monkeypatch):
    """The packed expansion also serves RigidBody{MRP} / RigidBody{RodriguesParam} with a compact cost block (DiagonalCost): the same six
    constant columns.  [A B] equal to the 4 x 16 kernel bit for bit, the cost block to one ulp, solves to 1e-9 with equal iteration counts;
    and equal to the oracle as before."""
    def mk(lib):
        model = T.Quadrotor(rotation=rot)
        n, m = model.dims()
        x0 = np.zeros(n); x0[:3] = [0.4, -0.3, 1.0]
        xf = np.zeros(n); xf[:3] = [0.0, 0.0, 1.5]
        obj = T.LQRObjective(np.full(n, 0.1), np.full(m, 0.01), np.full(n, 10.0), xf, 31)
        p = T.Problem(model, obj, x0, 1.0, xf=xf, lib=lib, batch=23)
        X0 = np.tile(x0, (23, 1)); X0[:, :3] += np.random.default_rng(6).uniform(-0.3, 0.3, (23, 3)); X0[:, 3:6] = np.random.default_rng(7).uniform(-0.1, 0.1, (23, 3))
        p.set_initial_state(X0)
        T.initial_controls(p, model.hover_control())
        return p
    out = []
    for pack in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_EXPAND_PACK", pack)
        p = mk(hip)
        perturb_controls((p,), 0.05)
        T.rollout(p); I.expand(p)
        A, Bm = I.dynamics_jacobians(p)
        ce = I.cost_expansion(p)
        s = T.iLQRSolver(p, iterations=25).solve()
        out.append((A, Bm, ce, s.stats["iterations"].copy(), T.states(p), T.controls(p)))
    np.testing.assert_array_equal(out[0][0], out[1][0]); np.testing.assert_array_equal(out[0][1], out[1][1])     # [A B]: bit for bit
    # the attitude block of the cost Hessian (the second-order term of the three-parameter error map) comes out of two different template
    # instantiations under hipcc's default FMA contraction: one ulp apart in a few entries (the quaternion model: none)
    for k in out[0][2]:
        np.testing.assert_allclose(out[0][2][k], out[1][2][k], rtol=4e-16, atol=1e-17, err_msg=k)
    np.testing.assert_array_equal(out[0][3], out[1][3])
    np.testing.assert_allclose(out[0][4], out[1][4], rtol=1e-9, atol=1e-11); np.testing.assert_allclose(out[0][5], out[1][5], rtol=1e-9, atol=1e-11)
    monkeypatch.setenv("TRAJOPT_EXPAND_PACK", "1")
    ph, po = mk(hip), mk(oracle)
    perturb_controls((ph, po), 0.05)
    for p in (ph, po):
        T.rollout(p); I.expand(p)
    Ah, Bh = I.dynamics_jacobians(ph); Ao, Bo = I.dynamics_jacobians(po)
    np.testing.assert_allclose(Ah, Ao, rtol=1e-9, atol=1e-11); np.testing.assert_allclose(Bh, Bo, rtol=1e-9, atol=1e-11)
    info = (ctypes.c_int32 * 8)()
    ph._call("solver_path", info)
    assert info[0] == 1          # MFMA backward pass: the tangent-matrix (packed) expansion ran


def test_solver_path_of_created_handles(hip, monkeypatch):
    """to_solver_path of freshly created handles (no solves) against rows of the table that tests/test_path_plan_host.py pins for the
    host-compiled path selection (csrc/path_plan.h; tests/host_shim/path_plan_harness.cpp ROWS, same names): what the built library
    reports is what the CPU-tested function decides.  Short horizons keep the large batches small; two rows have a knob set.  The
    thresholds scale with the compute units: the rows hold for 256 of them."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the pinned rows are those of a device with 256 compute units; this one has {cus}")
    cart = lambda B, con=False: configs.cartpole_problem(batch=B, N=11, tf=0.5, constrained=con, lib=hip)
    quad = lambda B: configs.quadrotor_problem(batch=B, N=11, tf=0.25, lib=hip)

    def hybrid():
        from test_hybrid_dims import hybrid_problem
        return hybrid_problem(hip, batch=200)[0]
    rows = [
        ("cartpole B1024 N11", lambda: cart(1024), {}, [0, 1, 0, 4, 2, 1, 1, 0]),
        ("cartpole B12288 N11 con0", lambda: cart(12288), {}, [0, 1, 0, 4, 2, 1, 1, 0]),
        ("cartpole B12288 N11 con1", lambda: cart(12288, True), {}, [2, 1, 1, 4, 2, 0, 1, 0]),
        ("cartpole B20480 N11 con0", lambda: cart(20480), {}, [2, 1, 1, 4, 2, 0, 1, 2]),
        ("cartpole B32768 N11 con1", lambda: cart(32768, True), {}, [2, 1, 1, 4, 2, 0, 1, 2]),
        ("quadrotor B4096 N11", lambda: quad(4096), {}, [1, 0, 1, 16, 2, 0, 1, 1]),
        ("hybrid B200", hybrid, {}, [0, 1, 0, 4, 2, 1, 1, 0]),
        ("cartpole B1024 SCAN=0", lambda: cart(1024), {"TRAJOPT_SCAN": "0"}, [0, 1, 0, 4, 2, 0, 1, 0]),
        ("quadrotor B4096 LS_REPACK=0", lambda: quad(4096), {"TRAJOPT_LS_REPACK": "0"}, [1, 0, 1, 16, 2, 0, 1, 0]),
    ]
    for name, make, env, want in rows:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            p = make()
        info = (ctypes.c_int32 * 8)()
        p._call("solver_path", info)
        assert list(info) == want, name
