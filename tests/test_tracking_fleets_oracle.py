"""tests/tracking_fleets.py on the CPU oracle alone: the inputs of tests/test_gpu_tracking_reference.py are vetted before a GPU sees them.

Each fleet, fed through N ``set_cost_linear_batch`` calls (the host recipe), must equal B single-trajectory oracle problems retargeted
with the existing 2-D ``T.update_trajectory``: integers exactly, X / U to 1e-12 (the batch evaluates c.q + (q_b - c.q), the single problem
q_b: one rounding apart).  And the fleets must be able to tell a per-trajectory reference from a shared one: against the solve in which
every trajectory tracks trajectory 0's reference, every other trajectory's states differ by more than 1e-2."""
import numpy as np
import pytest

import tracking_fleets as F


@pytest.mark.parametrize("name", sorted(F.FLEETS))
def test_fleet_equals_single_trajectory_problems(oracle, name):
    fleet = F.FLEETS[name]()
    singles = F.oracle_singles(name)
    p = fleet.problem(oracle)
    F.feed_by_recipe(p, fleet.Xref, fleet.Uref, fleet.start)
    got = F.solve(p, fleet)
    for k in F.INT_STATS:
        assert np.array_equal(got[k], singles[k]), k
    dx, du = np.abs(got["X"] - singles["X"]).max(), np.abs(got["U"] - singles["U"]).max()
    print(f"{name}: max |dX| {dx:.2e}, max |dU| {du:.2e}, iterations {got['iterations'].min()}..{got['iterations'].max()}")
    assert dx <= 1e-12 and du <= 1e-12, (dx, du)
    assert np.all(got["iterations"] >= 2), "the solves must iterate"


@pytest.mark.parametrize("name", sorted(F.FLEETS))
def test_fleet_tells_its_references_apart(oracle, name):
    fleet = F.FLEETS[name]()
    singles = F.oracle_singles(name)
    shared = F.solve(F.single_problem(fleet, oracle, 0), fleet)   # every start state is the same: trajectory 0's solve IS the shared-reference solve
    assert np.array_equal(fleet.x0, np.tile(fleet.x0[:1], (fleet.B, 1)))
    diff = np.abs(singles["X"] - shared["X"]).reshape(fleet.B, -1).max(axis=1)
    print(f"{name}: min over trajectories 1.. of max |X_b - X_0| = {diff[1:].min():.3e}; iterations differ for "
          f"{100.0 * np.mean(singles['iterations'][1:] != shared['iterations'][0]):.0f} %")
    assert diff[0] == 0.0
    assert np.all(diff[1:] > 1e-2), (int(np.argmin(diff[1:])) + 1, diff[1:].min())


def test_windows_and_shapes():
    for name, make in F.FLEETS.items():
        f = make()
        n, m = f.model.dims()
        assert f.Xref.shape == (f.B, f.Nref, n) and f.Uref.shape == (f.B, f.Nref, m) and f.start.shape == (f.B,) and f.start.dtype == np.int32
        assert f.start.min() >= 1 and (f.start - 1 + f.N).max() <= f.Nref, name          # every window fits: valid under "refuse"
        assert len(set(f.start.tolist())) > 1, name
        assert len(set(map(id, f.costs()))) == f.N                                       # a distinct cost per knot
    c, d, q = (F.FLEETS[k]() for k in ("cartpole", "double_integrator", "quadrotor"))
    assert (c.N, c.B, c.Nref) == (21, 70, 40) and (d.N, d.B) == (9, 65) and (q.N, q.B) == (11, 3)
    assert len(set(c.start[:64].tolist())) > 1 and c.B > 64 and d.B > 64                  # starts differ inside one 64-lane tile; a second tile
    assert np.all(q.costs()[0].Q[3:7] == 0.0)
    assert np.array_equal(F.window(np.array([1, 5]), 3, 6), [3, 5])
