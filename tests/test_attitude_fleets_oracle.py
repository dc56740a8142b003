"""Vets the fleets of tests/test_gpu_cost_attitude.py (tests/attitude_fleets.py) on the CPU oracle alone, before the HIP library is held to
them: B = 24 single-trajectory problems, each with its own attitude reference(s) in its DiagonalQuatCost descriptors.  At least 90 % of
every fleet ends SOLVE_SUCCEEDED under each solver the GPU tests use (the cap of tests/test_cost_weight_fleets_oracle.py); the attitude
matters — the same singles with the shared (goal fleet) or identity (tracking fleet) q_ref end on states that differ by a median above
1e-2; and no trajectory sits on a decision boundary of the solver: every integer output survives a move of the start state and the control
guess by one unit in the last place, in either direction, and the oracle's own answer moves by less than half of what the parity tests
allow (the margin of tests/test_oracle_sensitivity.py) — the conditions under which the GPU comparison holds integers bit for bit."""
import numpy as np
import pytest

import trajopt_amd as T
import attitude_fleets as AF

B = 24


@pytest.mark.parametrize("solver", ["ilqr", "al", "altro"])
@pytest.mark.parametrize("name", ["goal", "tracking"])
def test_fleet_on_the_oracle(name, solver, oracle):
    ref = AF.reference_solve(name, B, solver)
    flat = AF.reference_solve(name, B, solver, attitude=False)
    ok = ref.stats["status"] == AF.OK
    dX = AF.relerr(flat.X, ref.X)
    print(f"\n{name} B={B} {solver}: {100 * ok.mean():.1f} % succeeded (statuses {np.unique(ref.stats['status'])}), iterations "
          f"{ref.stats['iterations'].min()} .. {ref.stats['iterations'].max()}; without the per-trajectory attitude the states move by a median of {np.median(dX):.2e}")
    assert ok.mean() >= 0.9
    assert np.median(dX) > 1e-2                      # the attitude matters: a library that ignored the array would be seen
    assert len(np.unique(ref.stats["iterations"])) > 3
    if solver != "ilqr":
        assert ref.stats["c_max"][ok].max() < (1e-4 if solver == "al" else 1e-6)
        if solver == "altro":
            assert ref.stats["iterations_pn"].max() >= 1
    for ulps in (1, -1):   # no trajectory within rounding of a tie: the integers are comparable bit for bit
        nd = AF.reference_solve(name, B, solver, ulps=ulps)
        for k in AF.INTEGERS:
            moved = np.flatnonzero(nd.stats[k] != ref.stats[k])
            assert moved.size == 0, f"trajectories {moved} change their {k} under {ulps:+d} ulp"
        own = np.maximum(AF.relerr(nd.X, ref.X), AF.relerr(nd.U, ref.U))
        print(f"  {ulps:+d} ulp: the oracle's own answer moves by <= {own.max():.2e} (trajectory {own.argmax()})")
        assert own.max() < 0.5 * AF.solve_rtol(name, B, solver)


def test_fleets_are_what_the_issue_draws(oracle):
    for Bt in (24, 70):
        g = AF.goal(Bt)
        q = g.Xf[:, 3:7]
        np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, rtol=1e-14)
        assert np.all(np.abs(q) > 1e-4) and len(np.unique(q.round(12))) == q.size         # four non-zero components that differ by trajectory
        ang = np.degrees(2 * np.arccos(q[:, 0]))
        assert ang.min() >= 45.0 - 1e-9 and ang.max() <= 180.0 + 1e-9
        assert np.abs(g.Xf[:, :3] - g.xf[:3]).max() <= 0.5 and np.all(g.Xf[:, 7:] == 0.0)
        assert np.all(g.Q0[3:7] == 0.0) and np.all(g.Qf0[3:7] == 0.0)                      # the attitude goal lives in w min(1 +- q_ref'q) alone
        t = AF.tracking(Bt)
        assert t.Xref.shape == (Bt, 30, 13) and t.Uref.shape == (Bt, 30, 4) and t.start.min() >= 1 and t.start.max() <= 20
        assert (t.start - 1 + t.N - 1 > t.Nref - 1).any()                                  # some windows run past the end: HOLD clamps
        np.testing.assert_allclose(np.linalg.norm(t.Xref[:, :, 3:7], axis=2), 1.0, rtol=1e-14)
        np.testing.assert_allclose(t.Xref[:, 0, :3], t.x0[:, :3], atol=1e-14)                    # every helix passes through its trajectory's start position
        dt = t.tf / (t.N - 1)
        np.testing.assert_allclose(np.diff(t.Xref[:, :, 2], axis=1) / dt, t.Xref[:, 1:, 9], atol=1e-12)   # consistent climb
        assert np.all(t.Qd[3:7] == 0.0)
        p = t.problem(oracle, rows=[0])
        assert len(p._cost_objs) == t.N and all(c.kind == T.capi.COST_DIAGONAL_QUAT for c in p._cost_objs)


def test_single_carries_the_goal_attitude_and_the_nominal_constant(oracle):
    """The singles are what the issue's semantics describe: the nominal problem with q = -Q xf_b and q_ref = xf_b[q_ind]; c untouched."""
    g = AF.goal(B)
    p, nom = g.single(oracle, 3), g.shared(oracle, batch=1, b_offset=3)
    for c, c0, W in zip(p._cost_objs, nom._cost_objs, (g.Q0, g.Qf0)):
        np.testing.assert_array_equal(c.q_ref, g.Xf[3, 3:7]); np.testing.assert_array_equal(c.q, -W * g.Xf[3])
        assert c.c == c0.c and c.w == 1.0
        np.testing.assert_array_equal(c0.q_ref, g.xf[3:7])
    np.testing.assert_array_equal(p.x0, nom.x0)
    t = AF.tracking(B)
    s = t.single(oracle, 5)
    j = t.window(t.start[5], np.arange(t.N))
    assert j.max() == t.Nref - 1 or t.start[5] + t.N - 1 <= t.Nref
    for k, c in enumerate(s._cost_objs):
        np.testing.assert_array_equal(c.q_ref, t.Xref[5, j[k], 3:7]); np.testing.assert_array_equal(c.q, -t.W(k) * t.Xref[5, j[k]])


def test_combination_fleet_on_the_oracle(oracle):
    """Attitudes, weights, goals and control limits all per trajectory (the goal fleet, B = 24, ALTRO): the singles succeed, and integers and
    answers survive +-1 ulp on the inputs."""
    ref = AF.combo_reference("altro")
    ok = ref.stats["status"] == AF.OK
    print(f"\ncombination altro: {100 * ok.mean():.1f} % succeeded, iterations {ref.stats['iterations'].min()} .. {ref.stats['iterations'].max()}")
    assert ok.mean() >= 0.9 and len(np.unique(ref.stats["iterations"])) > 3
    for ulps in (1, -1):
        nd = AF.combo_reference("altro", ulps)
        for k in AF.INTEGERS:
            assert np.array_equal(nd.stats[k], ref.stats[k]), (k, np.flatnonzero(nd.stats[k] != ref.stats[k]))
        own = np.maximum(AF.relerr(nd.X, ref.X), AF.relerr(nd.U, ref.U))
        print(f"combination altro {ulps:+d} ulp: the oracle's own answer moves by <= {own.max():.2e}")
        assert own.max() < 0.5 * 1e-6
