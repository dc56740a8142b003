"""Vets the fleets of tests/test_gpu_model_params_instances.py (tests/model_params_fleet.py FLEETS, DEEP) on the CPU oracle alone, before any
flagged kernel instance is held to them — the way tests/test_failure_cases_oracle.py vets the failing batches: the solves succeed, the
trajectories of a fleet finish at different iterations (so a kernel that reads another trajectory's plant changes integers, not only
values), the polish runs and reaches the tolerance, the deep-search fleet does search deep and does fail somewhere, and the plants change
the trajectories by far more than the parity tolerance.  The seeds in FLEETS were fixed after these conditions held."""
import numpy as np
import pytest

import trajopt_amd as T
import model_params_fleet as F

OK = T.capi.SOLVE_SUCCEEDED
GOAL_PINNED = ("_con",)          # a GoalConstraint pins the terminal state: compare a mid-horizon knot instead


@pytest.mark.parametrize("name", list(F.FLEETS))
def test_solve_fleet(name, oracle):
    kind = F.FLEETS[name][0]
    fl = F.named_fleet(name, oracle)
    st = fl.stats
    counts = np.unique(st["iterations"])
    k = fl.X.shape[1] // 2 if kind.endswith(GOAL_PINNED) else -1
    spread = np.ptp(fl.X[:, k, :], axis=0).max()
    print(f"\n{name}: {100 * (st['status'] == OK).mean():.0f} % succeeded, {len(counts)} distinct iteration counts ({counts.min()}..{counts.max()}), "
          f"pn {st['iterations_pn'].min()}..{st['iterations_pn'].max()}, c_max {st['c_max'].max():.1e}, spread at knot {k}: {spread:.2e}")
    assert (st["status"] == OK).mean() >= 0.9
    assert len(counts) > 3
    assert spread > 1e-3
    if name in F.POLISHED:
        assert st["iterations_pn"].max() >= 1 and st["c_max"].max() <= 1e-6


def test_deep_search_fleet(oracle):
    kind, B, seed, kw = F.DEEP
    fl = F.fleet(kind, oracle, B, seed, **kw)
    ls = fl.ls_loop
    assert ls.shape == (kw["loop"], B) and fl.Jn_loop.shape == ls.shape
    print(f"\ndeep searches: {int((ls >= 4).sum())} of {ls.size} with index >= 4, {int((ls >= 8).sum())} with index >= 8, {int((ls < 0).sum())} failed")
    assert (ls >= 4).sum() > 100 and (ls < 0).sum() >= 1
    assert np.ptp(fl.X_loop[:, fl.X_loop.shape[1] // 2, :], axis=0).max() > 1e-3


def test_phase_fleets_differ(oracle):
    """The phases fleets of the ragged batches (B = 130, N = 11; smaller batches are its first trajectories: the generator fills the
    parameters row by row) and of every double-integrator dimension: the rolled-out terminal states differ."""
    assert all(a.params() == b.params() for a, b in zip(F.draw_models("cartpole", 63, 99), F.draw_models("cartpole", 130, 99)))
    fl = F.fleet("cartpole", oracle, 130, 99, phases=True, N=11, tf=0.5)
    assert np.ptp(fl.Xr[:, -1, :], axis=0).max() > 1e-3
    for D in (1, 2, 3):
        fl = F.named_fleet(f"dint{D}_con", oracle, phases=True)
        assert fl.Xr.shape == (70, 31, 2 * D) and np.ptp(fl.Xr[:, -1, :], axis=0).max() > 1e-3


def test_linear_fleet(oracle):
    fl, models, bv = F.linear_fleet(oracle, 70, F.LINEAR_SEED)
    st = fl.stats
    counts = np.unique(st["iterations"])
    print(f"\nlinear: {100 * (st['status'] == OK).mean():.0f} % succeeded, {len(counts)} distinct iteration counts, c_max {st['c_max'].max():.1e}")
    assert (st["status"] == OK).mean() >= 0.9 and len(counts) > 3
    assert np.ptp(fl.X[:, fl.X.shape[1] // 2, :], axis=0).max() > 1e-3
    c0 = fl.X[:, :-1, 0] - 0.5 * fl.X[:, :-1, 1] - bv[:, None, 0]
    c1 = fl.U[:, :, 0] + 2 * fl.U[:, :, 1] - bv[:, None, 1]
    assert max(c0.max(), c1.max()) < 2e-6                      # every trajectory inside ITS half-planes (the bound of tests/test_goal_batch.py)
