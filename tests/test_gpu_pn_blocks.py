"""The projected-Newton polish (csrc/k_pn.h) on the GPU away from the shapes it was tuned at: the ladder of block strides and the exit
cases of tests/pn_cases.py — vetted on the oracle by tests/test_pn_cases_oracle.py, run through the host build of the kernel source
by tests/test_pn_host.py — against the CPU oracle, through to_pn_solve and to_altro_solve; batch independence of the healthy
trajectories bit for bit; the refusal beyond the limits; one plant per trajectory; guard mode.  No trajectory is excluded anywhere."""
import ctypes as C

import numpy as np
import pytest

import trajopt_amd as T
import pn_cases as P
from test_gpu_parity import assert_trajectories_close

pytestmark = pytest.mark.gpu

_refs = {}


def reference(name, oracle):
    """the oracle's polish of a case, computed once and left unchanged"""
    if name not in _refs:
        _refs[name] = P.CASES[name].polish(oracle)
    return _refs[name]


def _compare(name, hip, oracle):
    case = P.CASES[name]
    ref = reference(name, oracle)
    ph = case.build(hip)
    NB, nb, _ = P.strides(case, ph)                      # the rung is hit on the device's own constraint values too
    assert NB == case.NB and int(nb.max()) == case.nb
    np.testing.assert_allclose(T.dynamics_defect(ph), T.dynamics_defect(case.build(oracle)), rtol=1e-9, atol=1e-13, equal_nan=True)
    got = case.polish(hip)
    for k in ("iterations",):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    P.assert_case_matches(case, got, ref, "gpu")
    return got, ref


@pytest.mark.parametrize("name", P.LADDER)
def test_ladder_vs_oracle(name, hip, oracle):
    """to_pn_solve on every rung of the ladder: status and projections bit-exact, X / U / c_max / cost / defect at the tolerances of
    test_gpu_pn.py::test_pn_solve_vs_oracle, every trajectory within constraint_tolerance"""
    got, _ = _compare(name, hip, oracle)
    assert np.all(got["status"] == T.capi.SOLVE_SUCCEEDED) and np.all(got["iterations_pn"] >= 1)
    assert got["c_max"].max() <= 1e-6 and got["defect"].max() <= 1e-6


@pytest.mark.parametrize("name", P.EXITS)
def test_exit_cases_vs_oracle(name, hip, oracle):
    """every exit of pn_begin / pn_project next to healthy trajectories: integers bit-exact, c_max NaN where the oracle's is NaN,
    the PROJECTION_FAIL trajectories at the tolerance the oracle's own spread sets (pn_cases.TOL)"""
    got, ref = _compare(name, hip, oracle)
    assert np.array_equal(np.isnan(got["c_max"]), np.isnan(ref["c_max"]))


@pytest.mark.parametrize("name", [n for n in P.EXITS if P.CASES[n].tol is not None])
def test_healthy_trajectories_do_not_see_the_failing_ones(name, hip, oracle):
    """bit for bit: the healthy trajectories of a mixed batch equal the same trajectories polished in a batch without the failing ones"""
    case = P.CASES[name]
    healthy = np.where(reference(name, oracle)["status"] == T.capi.SOLVE_SUCCEEDED)[0]
    assert 0 < healthy.size < case.B
    mixed, alone = case.polish(hip), case.polish(hip, sel=healthy)
    for k in ("X", "U", "iterations_pn", "c_max", "status"):
        np.testing.assert_array_equal(mixed[k][healthy], alone[k], err_msg=k)


@pytest.mark.parametrize("name", list(P.ALTRO))
def test_exit_cases_through_altro(name, hip, oracle):
    """the same through to_altro_solve (AL stage, then the polish with the case's options): integers bit-exact, values at the 1e-6 of
    test_gpu_pn.py::test_altro_solve_vs_oracle, c_max NaN where the oracle's is NaN — the trajectory with the NaN control is left
    alone by both stages — and the others equal, bit for bit, the batch without it"""
    case = P.CASES[name]
    nanc = P.ALTRO[name]
    got, ref = P.altro(case, hip, nan_control=nanc), P.altro(case, oracle, nan_control=nanc)
    for k in ("iterations", "iterations_outer", "iterations_pn", "status"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert np.array_equal(np.isnan(got["c_max"]), np.isnan(ref["c_max"]))
    fin = ~np.isnan(ref["c_max"])
    assert got["iterations_pn"].max() >= 1
    np.testing.assert_allclose(got["cost"][fin], ref["cost"][fin], rtol=1e-6)
    np.testing.assert_allclose(got["c_max"][fin], ref["c_max"][fin], rtol=1e-2, atol=1e-8)
    assert_trajectories_close(got["X"][fin], ref["X"][fin], 1e-6, "X")
    assert_trajectories_close(got["U"][fin], ref["U"][fin], 1e-6, "U")
    if nanc is not None:
        keep = np.where(fin)[0]
        alone = P.altro(case, hip, sel=keep)
        for k in ("X", "U", "iterations", "iterations_pn", "c_max", "status"):
            np.testing.assert_array_equal(got[k][keep], alone[k], err_msg=k)


@pytest.mark.parametrize("case", P.beyond_cases(), ids=lambda c: c.name)
def test_beyond_the_limits(case, hip, oracle):
    """One row more than the polish takes: to_pn_solve is refused as TO_ERR_UNSUPPORTED with the row limit in the message and the handle
    stays usable; to_altro_solve succeeds, polishes nothing, says so in to_last_error() and returns the AL stage's result unchanged."""
    L = P.limits()
    n, m = case.model.dims()
    ne = case.model.errstate_dim
    ph = case.build(hip)
    assert P.strides(case, ph)[0] == case.NB and (case.NB > L["nb_limit"] or case.NB - ne > L["max_rows"])
    X0, U0 = T.states(ph), T.controls(ph)
    with pytest.raises(T.UnsupportedError, match=f"more than {min(L['max_rows'], L['nb_limit'] - ne)} constraint rows on one knot"):
        T.ProjectedNewtonSolver(ph).solve()
    np.testing.assert_array_equal(T.states(ph), X0)       # nothing was touched, and the handle goes on answering
    np.testing.assert_array_equal(T.controls(ph), U0)
    assert np.all(np.isfinite(T.max_violation(ph)))
    # ... and a fresh handle whose constraint set fits is polished correctly (a descriptor keeps its row count under to_set_constraint,
    # so the refused handle cannot shed a row): the rung at the limit
    if case.name.startswith("quadrotor"):
        at = P.CASES[f"quadrotor_NB{L['nb_limit']}"]
        got = at.polish(hip)
        P.assert_case_matches(at, got, reference(at.name, oracle), "gpu, after the refusal")
    pa = case.build(hip)
    sa = T.ALTROSolver(pa).solve()
    assert hip.last_error().startswith("polish skipped:"), hip.last_error()
    assert np.all(sa.stats["iterations_pn"] == 0)
    o = P._options_of(pa)
    pb = case.build(hip)
    sb = T.ALSolver(pb, constraint_tolerance=o.projected_newton_tolerance).solve()
    assert np.any((sb.stats["status"] == T.capi.SOLVE_SUCCEEDED) & (sb.stats["c_max"] > o.constraint_tolerance)), "nothing was left to polish"
    for k in ("status", "c_max", "iterations", "iterations_outer"):
        np.testing.assert_array_equal(sa.stats[k], sb.stats[k], err_msg=k)
    np.testing.assert_array_equal(T.states(pa), T.states(pb))
    np.testing.assert_array_equal(T.controls(pa), T.controls(pb))


@pytest.mark.parametrize("name", list(P.FLEET))
def test_one_plant_per_trajectory(name, hip, oracle):
    """set_model_params: the PM instances of the polish (csrc/ops_plants_pn.hip) at a generic-path stride against B single-trajectory
    oracle problems, each on its own Cartpole"""
    case = P.CASES[name]
    models = P.fleet_models(case)
    ref = P.polish_fleet(case, oracle, models)
    ph = case.build(hip)
    T.set_model_params(ph, models)
    s = T.ProjectedNewtonSolver(ph).solve()
    got = dict(status=s.stats["status"], iterations_pn=s.stats["iterations_pn"], c_max=s.stats["c_max"], cost=s.stats["cost"],
               X=T.states(ph), U=T.controls(ph), defect=T.dynamics_defect(ph))
    P.assert_case_matches(case, got, ref, "gpu, one plant per trajectory")
    ok = ref["status"] == T.capi.SOLVE_SUCCEEDED
    assert ok.any() and got["c_max"][ok].max() <= 1e-6
    # the plants matter: on the shared model the same start ends elsewhere
    shared = case.polish(hip)
    assert np.abs(shared["X"][ok] - got["X"][ok]).max() > 1e-6


@pytest.mark.parametrize("name", P.GUARD)
def test_polish_runs_clean_under_the_guard(name, hip, monkeypatch):
    """TRAJOPT_GUARD=1: red zones around every device array of the handle, checked after the polish; same results as without"""
    out = []
    for guard in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_GUARD", guard)
        out.append(P.CASES[name].polish(hip))
    for k in ("X", "U", "status", "iterations_pn", "c_max"):
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
