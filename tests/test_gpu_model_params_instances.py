"""Per-trajectory plants on the flagged kernel instances tests/test_gpu_model_params_batch.py never launches: the run-time
integrator instances (RK3, Euler), the double integrator in one and three dimensions, the polish of the double integrators and the
Quadrotor, the constrained Quadrotor's forward variant, the Cartpole on the tangent-matrix layout, the repacked line-search rounds, and
plants together with per-trajectory goals and constraint parameters.  The reference is that file's: B single-trajectory ORACLE problems,
problem b on model b with trajectory b's start state (tests/model_params_fleet.py; every fleet used here is vetted on the oracle alone by
tests/test_model_params_fleets_oracle.py).  The tolerances are that file's too — rollout 1e-11 / 1e-12, Jacobians 1e-9 / 1e-11, gains rtol
1e-7 / atol 1e-9, line-search indices equal, J_new rtol 1e-10, cost rtol 1e-12; solves: assert_fleet_parity with 1e-4 for the trajectories
the oracle itself cut off.  Every handle is asserted onto the layout it claims through to_solver_path.  B = 70 unless said: two tiles,
the second with six live lanes."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import model_params_fleet as F
from test_gpu_model_params_batch import solver_path, _resolve, _solve_fresh
from test_gpu_parity import assert_trajectories_close

pytestmark = pytest.mark.gpu
OK = T.capi.SOLVE_SUCCEEDED
COOP, MFMA, LANE = 0, 1, 2
LAYOUT_ENV = {"coop": {}, "lane": {"TRAJOPT_BACKWARD": "lane"}, "mfma": {"TRAJOPT_BACKWARD": "mfma"}}


def setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def on_layout(p, flavour):
    """A handle with plants sits on the layout the test claims, with none of the kernels that have no flagged instance."""
    info = solver_path(p)
    assert info[0] == flavour and info[1] == 0 and info[5] == 0 and (info[7] & 2) == 0, info
    return info


def plant_problem(name, hip, flavour, B=None, models=None, goals=None, goals_first=False):
    """The batch problem of FLEETS[name] on the shared model with the fleet's models (and goals) set per trajectory."""
    kind, B0, seed, _, kw = F.FLEETS[name]
    B = B or B0
    models = F.draw_models(kind, B, seed) if models is None else models
    p = F.build(kind, hip, B, **F.build_kw(kw))
    goals = kw.get("goals") if goals is None else goals
    if goals is not None and goals_first:
        T.set_goal_state(p, goals)
    T.set_model_params(p, models)
    if goals is not None and not goals_first:
        T.set_goal_state(p, goals)
    on_layout(p, flavour)
    return p


def assert_phases(p, fl, sel=slice(None)):
    """The phases test of tests/test_gpu_model_params_batch.py: rollout, cost, discrete Jacobian, defect, A / B, gains, forward pass."""
    T.rollout(p)
    np.testing.assert_allclose(T.states(p), fl.Xr[sel], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(T.cost(p), fl.J[sel], rtol=1e-12)
    np.testing.assert_allclose(I.discrete_jacobian(p), fl.F[sel], rtol=1e-9, atol=1e-11)
    d = T.dynamics_defect(p)
    assert d.max() < 1e-12, d.max()                                              # each trajectory satisfies ITS OWN dynamics
    I.expand(p)
    A, Bm = I.dynamics_jacobians(p)
    np.testing.assert_allclose(A, fl.A[sel], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Bm, fl.Bm[sel], rtol=1e-9, atol=1e-11)
    I.backwardpass(p)
    g = I.gains(p)
    np.testing.assert_allclose(g["K"], fl.K[sel], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["d"], fl.d[sel], rtol=1e-7, atol=1e-9)
    ls, Jn = I.forwardpass(p)
    np.testing.assert_array_equal(ls, fl.ls[sel])
    np.testing.assert_allclose(Jn, fl.Jn[sel], rtol=1e-10)


def assert_solve(name, p, fl):
    _, _, _, solver, kw = F.FLEETS[name]
    s = F.SOLVERS[solver](p, **kw.get("solver_kw", {})).solve()
    assert (s.stats["status"] == OK).mean() >= 0.9
    F.assert_fleet_parity(s, p, fl, unconverged_rtol=1e-4)
    if solver == "altro":
        np.testing.assert_array_equal(s.stats["iterations_pn"], fl.stats["iterations_pn"])
        assert s.stats["iterations_pn"].max() >= 1 and s.stats["c_max"].max() <= 1e-6   # the polish ran, on each trajectory's own dynamics
    return s


def outputs(s, p):
    return [s.stats[k].copy() for k in ("status", "iterations", "iterations_outer", "iterations_pn", "cost", "c_max")] + [T.states(p), T.controls(p)]


def assert_identical(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------------ a. run-time integrator instances
#   k_rollout<M, -1, true>, k_expand<M, -1, 7, 0 / 1, false, true>, k_expand_lane<M, -1, 7, true>, k_forward<M, 40> (42 with the bounds of the
#   double integrator), k_discrete_jacobian / k_defect with the integrator read at run time
INTEGRATOR_CASES = [(f"{model}_{integ}", layout, flavour) for integ in ("rk3", "euler")
                    for model, layout, flavour in (("cartpole", "coop", COOP), ("cartpole", "lane", LANE), ("cartpole", "mfma", MFMA), ("dint", "coop", COOP),
                                                   ("quadrotor", "coop", MFMA))]


@pytest.mark.parametrize("name,layout,flavour", INTEGRATOR_CASES)
def test_integrator_phases(name, layout, flavour, hip, oracle, monkeypatch):
    setenv(monkeypatch, LAYOUT_ENV[layout])
    assert_phases(plant_problem(name, hip, flavour), F.named_fleet(name, oracle, phases=True))


@pytest.mark.parametrize("name,layout,flavour", INTEGRATOR_CASES)
def test_integrator_solves(name, layout, flavour, hip, oracle, monkeypatch):
    """iLQR solves (the double integrator carries control bounds: an AL solve, since its iLQR solves end at the same two iteration
    counts for every plant)."""
    setenv(monkeypatch, LAYOUT_ENV[layout])
    assert_solve(name, plant_problem(name, hip, flavour), F.named_fleet(name, oracle))


def test_cartpole_rk3_altro(hip, oracle):
    """MODE 42 with the integrator read at run time, then the polish (k_pn_* with PM) on RK3 defects."""
    assert_solve("cartpole_con_rk3", plant_problem("cartpole_con_rk3", hip, COOP), F.named_fleet("cartpole_con_rk3", oracle))


# ------------------------------------------------------------------------------------------------ b. D = 1, 2, 3
DINT_CASES = [(1, "coop", COOP), (1, "lane", LANE), (2, "coop", COOP), (2, "lane", LANE), (3, "coop", COOP)]   # (D = 3 has no lane layout)


@pytest.mark.parametrize("D,layout,flavour", DINT_CASES)
def test_double_integrator_dimensions(D, layout, flavour, hip, oracle, monkeypatch):
    """Every flagged instance of DoubleIntegratorModel<D>: phases, then an ALTRO solve with bounds and a goal constraint (polished)."""
    setenv(monkeypatch, LAYOUT_ENV[layout])
    name = f"dint{D}_con"
    assert_phases(plant_problem(name, hip, flavour), F.named_fleet(name, oracle, phases=True))
    assert_solve(name, plant_problem(name, hip, flavour), F.named_fleet(name, oracle))


@pytest.mark.parametrize("integration", [T.RK4, T.RK3])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_unconstrained_double_integrator_phases(D, integration, hip, oracle):
    """k_forward<DoubleIntegratorModel<D>, 44> (RK4) and <…, 40> (RK3): the forward variants without constraint terms, which the bounded
    fleets above never launch; with RK3 also the run-time integrator instances of the rollout and the expansion for D = 1 and 3."""
    kw = dict(D=D, integration=integration)
    p = F.build("dint_free", hip, 70, **kw)
    T.set_model_params(p, F.draw_models("dint_free", 70, 89, D=D))
    on_layout(p, COOP)
    fl = F.fleet("dint_free", oracle, 70, 89, phases=True, **kw)
    assert np.ptp(fl.Xr[:, -1, :], axis=0).max() > 1e-3
    assert_phases(p, fl)


@pytest.mark.parametrize("D,layout,flavour", DINT_CASES)
def test_double_integrator_rollout_is_its_taylor_series(D, layout, flavour, hip, monkeypatch):
    """A reference that is not the oracle: RK4 of a double integrator is its exact Taylor series, x+ = A x + B(m_b) u with A = [I hI; 0 I],
    B = [h^2 / 2 m_b I; h / m_b I] (tests/test_hybrid_dims.py lqr_reference), applied to the kernel's own X[b, k].  1e-13 in
    assert_trajectories_close's measure (against the trajectory's largest entry): x + h v + h^2 / 2m u cancels for some entries, and
    the rounding of both sides is relative to the largest term of that sum, not to the sum."""
    setenv(monkeypatch, LAYOUT_ENV[layout])
    name = f"dint{D}_con"
    kind, B, seed, _, _ = F.FLEETS[name]
    models = F.draw_models(kind, B, seed)
    p = plant_problem(name, hip, flavour)
    U = np.random.default_rng(seed).uniform(-2.0, 2.0, (B, p.N - 1, D))
    T.initial_controls(p, U)
    T.rollout(p)
    X = T.states(p)
    h = p.tf / (p.N - 1)
    mass = np.array([mod.mass for mod in models])[:, None, None]
    want = np.concatenate([X[:, :-1, :D] + h * X[:, :-1, D:] + h * h / (2 * mass) * U, X[:, :-1, D:] + h / mass * U], axis=2)
    assert np.ptp(mass) > 0.3
    assert_trajectories_close(X[:, 1:], want, 1e-13, "X")


# ------------------------------------------------------------------------------------------------ c. Cartpole, tangent-matrix layout
def test_cartpole_tangent_matrix_layout(hip, oracle, monkeypatch):
    """k_expand<CartpoleModel, *, 7, 1, false, true> (TRAJOPT_BACKWARD=mfma).  The compact cost block is off: launch_expand refuses a
    handle with plants and h_compact by name, so every expansion below shows it.  Then clear_model_params: the re-solve equals a fresh
    shared handle under the same knob bit for bit (the constant columns are rewritten)."""
    setenv(monkeypatch, LAYOUT_ENV["mfma"])
    kw = dict(N=41, tf=1.0)
    p = F.build("cartpole", hip, 70, **kw)
    T.set_model_params(p, F.draw_models("cartpole", 70, 21))
    on_layout(p, MFMA)
    assert_phases(p, F.fleet("cartpole", oracle, 70, 21, phases=True, **kw))       # (the phases fleet of test_gpu_model_params_batch.py)
    p = plant_problem("cartpole_rk4", hip, MFMA)
    assert_solve("cartpole_rk4", p, F.named_fleet("cartpole_rk4", oracle))
    assert_solve("cartpole_con_al", plant_problem("cartpole_con_al", hip, MFMA), F.named_fleet("cartpole_con_al", oracle))
    T.clear_model_params(p)
    assert solver_path(p)[0] == MFMA
    for got, want in zip(_resolve(p, "cartpole"), _solve_fresh("cartpole", hip, 70)):
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ d. repacked line-search rounds
def deep_loop(hip, monkeypatch, repack, models, x0=None):
    kind, B, seed, kw = F.DEEP
    monkeypatch.setenv("TRAJOPT_LS_REPACK", repack)
    p = F.build(kind, hip, B, x0=x0, **F.build_kw(kw))
    T.set_model_params(p, models)
    info = on_layout(p, MFMA)
    assert (info[7] & 1) == int(repack), info
    return F.phase_loop(p, kw["loop"])


def test_deep_line_searches_in_repacked_rounds(hip, oracle, monkeypatch):
    """k_forward<QuadrotorModel, 42> with four candidates per round: in a repacked round a lane rolls out ANOTHER lane's trajectory and
    must do so on that trajectory's plant.  Thirty rounds of expand / backward pass / forward pass with a dual update every tenth,
    against the fleet's: every round's indices equal, J_new at 1e-10; more than 100 searches go past the first round.  The same loop
    on the static lane map (TRAJOPT_LS_REPACK=0) is bit-identical (the rule of test_line_search_repack), and with a common start state
    the reversed plants give the reversed results bit for bit."""
    kind, B, seed, kw = F.DEEP
    monkeypatch.setenv("TRAJOPT_LS_DEEP", "0")
    monkeypatch.setenv("TRAJOPT_LS_CANDIDATES", "4")
    fl = F.fleet(kind, oracle, B, seed, **kw)
    models = F.draw_models(kind, B, seed)
    ls, Jn, X, U = deep_loop(hip, monkeypatch, "1", models)
    for it in range(kw["loop"]):
        np.testing.assert_array_equal(ls[it], fl.ls_loop[it], err_msg=f"round {it}")
        np.testing.assert_allclose(Jn[it], fl.Jn_loop[it], rtol=1e-10, err_msg=f"round {it}")
    assert_trajectories_close(X, fl.X_loop, 1e-6, "X")
    assert_trajectories_close(U, fl.U_loop, 1e-6, "U")
    assert ((ls >= 4) | (ls < 0)).sum() > 100, "the searches never went past the first round"
    assert_identical((ls, Jn, X, U), deep_loop(hip, monkeypatch, "0", models))
    x0 = np.r_[np.zeros(3), 1.0, np.zeros(9)]
    fwd, rev = deep_loop(hip, monkeypatch, "1", models, x0=x0), deep_loop(hip, monkeypatch, "1", models[::-1], x0=x0)
    assert np.ptp(fwd[2][:, -1, :], axis=0).max() > 1e-3                              # the plants alone make them differ
    assert_identical(fwd, (rev[0][:, ::-1], rev[1][:, ::-1], rev[2][::-1], rev[3][::-1]))


# ------------------------------------------------------------------------------------------------ e. Quadrotor ALTRO
def test_quadrotor_altro(hip, oracle, monkeypatch):
    """k_forward<QuadrotorModel, 42> in a solve with compaction, then k_pn_begin / k_pn_lin_col / k_pn_project<QuadrotorModel, true>;
    a guarded run (TRAJOPT_GUARD=1) is bit-identical."""
    out = []
    for guard in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_GUARD", guard)
        p = plant_problem("quadrotor_con", hip, MFMA)
        assert solver_path(p)[2] == 1
        s = assert_solve("quadrotor_con", p, F.named_fleet("quadrotor_con", oracle))
        out.append(outputs(s, p))
    assert_identical(*out)


# ------------------------------------------------------------------------------------------------ f. with the other per-trajectory inputs
@pytest.mark.parametrize("name,layout,flavour", [("cartpole_goals", "coop", COOP), ("cartpole_goals", "lane", LANE), ("quadrotor_goals", "coop", MFMA),
                                                 ("cartpole_con_goals", "coop", COOP), ("cartpole_con_goals", "lane", LANE)])
def test_plants_and_goals_per_trajectory(name, layout, flavour, hip, oracle, monkeypatch):
    """B goals (`gl`; GoalConstraint targets `cp` for cartpole_con) on top of B plants; oracle problem b has model b and the scalar
    set_goal_state(p, Xf[b]).  Goals then plants equals plants then goals bit for bit."""
    setenv(monkeypatch, LAYOUT_ENV[layout])
    fl = F.named_fleet(name, oracle)
    out = []
    for goals_first in (False, True):
        p = plant_problem(name, hip, flavour, goals_first=goals_first)
        out.append(outputs(assert_solve(name, p, fl), p))
    assert_identical(*out)
    assert np.ptp(F.FLEETS[name][4]["goals"][:, 0]) > 0.5                       # (the goals do differ)


def test_plants_and_linear_right_hand_sides_per_trajectory(hip, oracle):
    """One LinearConstraint right-hand side per trajectory (set_constraint_params_batch) on top of B plants: linear_problem's model is
    the 2-D double integrator, one of the three supported.  Either order of the two setters gives the same bits."""
    from test_goal_batch import linear_problem
    B = 70
    fl, models, bv = F.linear_fleet(oracle, B, F.LINEAR_SEED)
    out = []
    for rhs_first in (False, True):
        p, _ = linear_problem(hip, B, bv if rhs_first else None)
        T.set_model_params(p, models)
        if not rhs_first:
            T.set_constraint_params_batch(p, 0, bv)
        on_layout(p, COOP)
        s = T.ALSolver(p).solve()
        F.assert_fleet_parity(s, p, fl, unconverged_rtol=1e-4)
        out.append(outputs(s, p))
    assert_identical(*out)
    X, U = out[0][6], out[0][7]
    assert max((X[:, :-1, 0] - 0.5 * X[:, :-1, 1] - bv[:, None, 0]).max(), (U[:, :, 0] + 2 * U[:, :, 1] - bv[:, None, 1]).max()) < 2e-6


# ------------------------------------------------------------------------------------------------ g. ragged batches
@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_ragged_batches_on_the_lane_layout(B, hip, oracle, monkeypatch):
    """One trajectory (the spare tile only), a tile less one, a tile and one, two tiles and two: the first B trajectories of one fleet."""
    setenv(monkeypatch, LAYOUT_ENV["lane"])
    kw = dict(N=11, tf=0.5)
    fl = F.fleet("cartpole", oracle, 130, 99, phases=True, **kw)
    p = F.build("cartpole", hip, B, **kw)
    T.set_model_params(p, F.draw_models("cartpole", 130, 99)[:B])
    on_layout(p, LANE)
    assert_phases(p, fl, slice(0, B))
