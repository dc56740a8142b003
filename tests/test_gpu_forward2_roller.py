"""The roller of the two-wave forward pass (k_forward.h fwd2_roll) against the one-wave kernel, bit for bit.

For the models whose gains row travels in registers the roller's knot loop is unrolled by two: knot data and state ping-pong between
two register sets, the ring slot k & 1 is a constant of each half, and a horizon with an odd number of stage knots ends in a tail
knot.  Nothing of that may change a bit of what k_forward computes, so every test here drives rollout -> expand -> backwardpass ->
forwardpass through the phase API once with TRAJOPT_FWD2=0 (k_forward) and once with =1 (k_forward2) and compares line-search
indices, J, X and U for equality: horizons with N - 1 = 1 (no loop pass), 2 and 4 (whole passes), 3 (a pass and the tail); one lane,
a partly filled wave and a second workgroup; line searches that reuse the ring over several rounds of one launch; a second
registers-gains model with another ring slot size; and the LDS-gains instance (Quadrotor), which keeps the rolled loop."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

pytestmark = pytest.mark.gpu


def drive_both(build, monkeypatch, iterations, dual_update_at=None):
    """`iterations` iLQR iterations on two handles of the same problem, one per kernel; every output compared for equality after each.
    Returns the line-search indices of all iterations [iterations, B]."""
    probs = []
    for two in ("0", "1"):
        monkeypatch.setenv("TRAJOPT_FWD2", two)
        p = build()
        T.rollout(p)
        probs.append(p)
    indices = []
    for it in range(iterations):
        out = []
        for p in probs:
            if dual_update_at is not None and it == dual_update_at:
                I.dual_update(p)
            I.expand(p); I.backwardpass(p)
            ls, J = I.forwardpass(p)
            out.append((np.array(ls).copy(), np.array(J).copy(), T.states(p), T.controls(p)))
        (l0, J0, X0, U0), (l1, J1, X1, U1) = out
        np.testing.assert_array_equal(l1, l0, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(J1, J0, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(X1, X0, err_msg=f"iteration {it}")
        np.testing.assert_array_equal(U1, U0, err_msg=f"iteration {it}")
        assert np.all(np.isfinite(J0)) and np.all(np.isfinite(X0))
        indices.append(l0)
    return np.array(indices)


def cartpole(batch, N, hip, swing=False):
    """Short-horizon Cartpoles.  swing: time steps of 0.6 s and a hard push as the initial guess — far from linear, so that the first step
    sizes are rejected and the line search goes on (the later-rounds test; the CPU oracle backtracks 41 / 84 times in its six
    iterations at N = 4 / 5, up to step size 11, and never fails a search)."""
    def build():
        p = configs.cartpole_problem(batch=batch, N=N, tf=(0.6 if swing else 0.1) * (N - 1), lib=hip)
        if swing:
            T.initial_controls(p, np.array([8.0]))
        return p
    return build


@pytest.mark.parametrize("N", [2, 3, 4, 5])
def test_cartpole_horizons_and_batches(N, hip, monkeypatch):
    for batch in (1, 17, 65):
        drive_both(cartpole(batch, N, hip), monkeypatch, iterations=4)


@pytest.mark.parametrize("N", [4, 5])
def test_cartpole_later_line_search_rounds(N, hip, monkeypatch):
    """One step size per round and no deep shape: a trajectory that rejects the full step runs further rounds inside the same launch,
    each of which starts on ring slot 0 again."""
    monkeypatch.setenv("TRAJOPT_LS_CANDIDATES", "1")
    monkeypatch.setenv("TRAJOPT_LS_DEEP", "0")
    ls = drive_both(cartpole(17, N, hip, swing=True), monkeypatch, iterations=6)
    later_rounds = int((ls >= 1).sum())
    assert later_rounds > 10, later_rounds


@pytest.mark.parametrize("N", [2, 3, 4, 5])
def test_double_integrator_horizons(N, hip, monkeypatch):
    """2-D double integrator: n + 2 m = 8, four 16-byte pieces per ring slot (the Cartpole has three)."""
    def build():
        model = T.DoubleIntegrator(1.0, 2)
        obj = T.LQRObjective(np.array([1.0, 2.0, 0.5, 0.3]), np.array([0.1, 0.2]), 10 * np.ones(4), np.array([1.0, 2.0, 0, 0]), N)
        p = T.Problem(model, obj, np.array([0.2, -0.1, 0.0, 0.3]), 0.1 * (N - 1), batch=17, lib=hip)
        p.set_initial_state(np.linspace(-0.5, 0.5, 17)[:, None] * np.array([1.0, -1.0, 0.5, 0.25]))
        T.initial_controls(p, np.array([0.1, -0.05]))
        return p
    drive_both(build, monkeypatch, iterations=3)


@pytest.mark.parametrize("N", [4, 5])
def test_quadrotor_lds_gains_instance(N, hip, monkeypatch):
    """Constrained Quadrotor (gains staged through LDS by DMA): the roller keeps its rolled loop; both horizon parities."""
    def build():
        o = T.SolverOptions(lib=hip, constraint_tolerance=1e-4)
        return configs.quadrotor_problem(batch=5, N=N, tf=0.05 * (N - 1), constrained=True, lib=hip, options=o)
    drive_both(build, monkeypatch, iterations=5, dual_update_at=3)


def test_cartpole_whole_solve_two_wave(hip, oracle, monkeypatch):
    from test_gpu_parity import assert_solve_parity
    monkeypatch.setenv("TRAJOPT_FWD2", "1")
    ph, po = configs.cartpole_problem(batch=33, lib=hip), configs.cartpole_problem(batch=33, lib=oracle)
    sh, so = T.iLQRSolver(ph).solve(), T.iLQRSolver(po).solve()
    assert_solve_parity(sh, so, ph, po)
