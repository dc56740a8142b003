"""The fleets of tests/test_gpu_time_steps.py on the CPU oracle alone (tests/time_step_fleets.py): every solve fleet used on the GPU ends
SOLVE_SUCCEEDED for >= 90 % of its trajectories (the condition the GPU tests ask for, met here before any seed was fixed), and the
per-trajectory steps really matter — the results differ between the trajectories by far more than the parity tolerances, so a kernel that
read the shared step, dt[0] or a neighbour's would not pass."""
import numpy as np
import pytest

import trajopt_amd as T
import time_step_fleets as F

OK = T.capi.SOLVE_SUCCEEDED


def test_drawn_steps():
    for ragged in (False, True):
        dt = F.draw_steps(1.5, 31, 70, 5, ragged)
        assert dt.shape == (70, 30) and np.all(dt > 0)
        tf = dt.sum(axis=1)
        assert tf.min() > 1.5 * (1 - F.SPREAD_TF) * (1 - F.SPREAD_KNOT) and tf.max() < 1.5 * (1 + F.SPREAD_TF) * (1 + F.SPREAD_KNOT)
        if ragged:
            assert np.ptp(dt, axis=1).min() > 0.1 * dt.mean() and len(np.unique(dt)) == dt.size      # another grid per trajectory AND per knot
        else:
            assert np.all(dt[0] == 1.5 / 30) and np.all(np.ptp(dt, axis=1) == 0) and len(np.unique(dt[:, 0])) == 70
            np.testing.assert_array_equal(dt[:, 0], F.draw_final_times(1.5, 70, 5) / 30)


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "uniform"])
@pytest.mark.parametrize("case", list(F.SOLVES))
def test_solve_fleets_on_the_oracle(case, ragged, oracle):
    fl = F.solve_fleet(case, oracle, ragged)
    kind, B = F.SOLVES[case][:2]
    assert fl.B == B and (fl.stats["status"] == OK).mean() >= 0.9
    # the steps matter: iteration counts spread over many values, and (where no goal constraint pins it) so does the terminal state
    assert len(np.unique(fl.stats["iterations"])) >= 10
    if kind != "cartpole_con":
        assert np.ptp(fl.X[:, -1, :], axis=0).max() > 1e-2
    else:
        assert np.ptp(fl.U[:, 0, :], axis=0).max() > 1e-2 and fl.stats["iterations_pn"].max() >= 1 and fl.stats["c_max"].max() <= 1e-6


def test_combined_fleets_on_the_oracle(oracle):
    fl, models = F.plants_steps_fleet(oracle)
    assert (fl.stats["status"] == OK).mean() >= 0.9 and len(np.unique(fl.stats["iterations"])) >= 10 and len(models) == fl.B
    fb, a = F.bounds_steps_fleet(oracle)
    assert (fb.stats["status"] == OK).mean() >= 0.9 and len(np.unique(fb.stats["iterations"])) >= 5
    # the per-trajectory bounds bind: the largest control of a trajectory sits at ITS bound (AL tolerance 1e-4, held to 2e-4)
    umax = np.abs(fb.U).max(axis=(1, 2))
    assert np.all(umax <= a + 2e-4) and (umax >= a - 1e-3).mean() > 0.5 and np.ptp(a) > 0.3


@pytest.mark.parametrize("kind", list(F.PHASES))
def test_phase_fleets_on_the_oracle(kind, oracle):
    fl = F.phase_fleet(kind, oracle)
    assert np.ptp(fl.Xr[:, -1, :], axis=0).max() > 1e-2 and np.ptp(fl.J) > 1.0        # rollouts and costs differ
    assert fl.defect.max() < 1e-12 and fl.Jk.shape == (fl.B, 41)
    assert len(np.unique(fl.ls)) >= 2 or kind == "quadrotor"                          # (the Quadrotor's first step is accepted whole by all)


def test_phase_fleets_are_well_conditioned_on_the_oracle(oracle):
    """The J_new of the phase fleets is held to rtol 1e-10 on the GPU: the oracle's own J_new must not move by more than a tenth of that
    under a 1e-12 relative nudge of the control guess (what decided which fleet scales its stage costs by dt, time_step_fleets.PHASE_KW)."""
    from trajopt_amd import internal as I
    import model_params_fleet as M
    for kind in F.PHASES:
        kw = F.PHASE_KW[kind]
        dt, _ = F.steps_of(kind, 70, F.PHASES[kind], True, **kw)
        fl = F.phase_fleet(kind, oracle)
        for b in range(0, 70, 3):
            p = F.with_steps(M.build(kind, oracle, 1, b_offset=b, **kw), dt[b], oracle, options=kw.get("options"))
            T.initial_controls(p, T.controls(p) * (1 + 1e-12))
            T.rollout(p); I.expand(p); I.backwardpass(p)
            ls, Jn = I.forwardpass(p)
            assert ls[0] == fl.ls[b] and abs(Jn[0] - fl.Jn[b]) <= 1e-11 * abs(fl.Jn[b]), (kind, b, Jn[0], fl.Jn[b])
