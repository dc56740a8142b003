"""Re-solves on a RECONFIGURED handle (batched MPC: one handle, solved again and again with something changed in between) against a handle
without history and against the oracle.  A handle keeps state across solves that was sized or chosen for the configuration it had when the
state was first needed: the two repacked working sets and their maps, the per-trajectory cost terms and constraint parameters with their
flags, the polish workspace and its tables, the kernel variants the host picks while anything is flagged.  Every sequence here (definitions
and the runner: tests/test_handle_reuse_oracle.py check_sequence) runs differently configured solves on ONE handle; every step must equal,
bit for bit and over the whole batch, a newly created handle given the same configuration from scratch and the recorded start state, agree
with the oracle (all trajectories at small batch, a fixed sample of 512 at large — chosen on the CPU so that the asserts are hard), and give
the same bits again under TRAJOPT_GUARD=1."""
import numpy as np
import pytest

import trajopt_amd as T
from test_handle_reuse_oracle import LARGE, SMALL, check_sequence, sample_indices

pytestmark = pytest.mark.gpu


def _drains_unevenly(snap, B, what):
    """Several moves into a repacked working set happened: many distinct iteration counts, and at some batch step fewer than half of the batch
    was still iterating while more than 2 048 (TRAJOPT_REPACK) were."""
    it = snap["stats"]["iterations"]
    active = np.array([(it > k).sum() for k in range(int(it.max()) + 1)])
    assert len(set(it)) > 10, (what, sorted(set(it)))
    assert ((active > 2048) & (active < B / 2)).any(), (what, active)


@pytest.mark.parametrize("order", ["gl_cp", "cp_gl"])
def test_sequence_A_repacked_working_set_constrained_cartpole(order, hip, oracle, monkeypatch):
    """40 000 constrained Cartpoles, moves down to 2 048, iLQR with 25 iterations, warm starts: shared goal -> dual update, goals per trajectory on
    the costs only (the table of carried arrays gains gl) -> cleared, GoalConstraint target per trajectory (cp: the SAME number of carried arrays
    with other row lengths — a working set re-used by count wrote lam into the buffer sized for gl) -> both -> cleared; and with cp before gl.  The
    handle without history is created with TRAJOPT_REPACK=0: it has no working set at all."""
    seq = LARGE["A_" + order]()

    def per_step(i, step, start, snap, p):
        what = f"{seq.name} step {i} ({step.name})"
        path = snap["path"]
        assert path[0] == 2 and path[1] == 1 and path[7] & 2, "the constrained batch must take the fused lane path with a repacked working set"
        _drains_unevenly(snap, seq.B, what)
        if i == 1:
            lam = start["duals"][0][0]
            assert np.abs(lam).max() > 0 and np.ptp(np.abs(lam).reshape(seq.B, -1).max(axis=1)) > 0, "per-trajectory duals differ before the second solve"
    check_sequence(seq, hip, oracle, monkeypatch.setenv, sample=sample_indices(seq.B), fresh_env={"TRAJOPT_REPACK": "0"}, per_step=per_step)


def test_sequence_B_repacked_working_set_growing_first_move(hip, oracle, monkeypatch):
    """70 000 Cartpoles: a solve whose first move is small (90 % of the batch starts at the controls of an earlier solve, the rest cold) -> a cold
    start of the whole batch (first move large: both working sets and their maps must grow) -> goals per trajectory (the table gains gl) ->
    cleared."""
    seq = LARGE["B"]()
    first_moves = []

    def per_step(i, step, start, snap, p):
        _drains_unevenly(snap, seq.B, f"{seq.name} step {i} ({step.name})")
        assert snap["path"][7] & 2
        it = snap["stats"]["iterations"]
        active = np.array([(it > k).sum() for k in range(int(it.max()) + 1)])
        first_moves.append(int(active[active <= 0.7 * seq.B][0]))       # the first count the solve loop may move (TRAJOPT_REPACK_AT)
    check_sequence(seq, hip, oracle, monkeypatch.setenv, sample=sample_indices(seq.B), fresh_env={"TRAJOPT_REPACK": "0"}, per_step=per_step)
    assert first_moves[1] > 2 * first_moves[0], first_moves


@pytest.mark.parametrize("kind", ["cartpole", "cartpole_lane", "quadrotor"])
def test_sequence_C_kernel_variant_switches(kind, hip, oracle, monkeypatch):
    """ALTRO, shared goal -> ALTRO, goal per trajectory on costs and GoalConstraint -> AL, goals on the costs only -> cleared, iLQR on the AL solve's
    duals -> ALTRO again: the host must return to the default kernel variants (solver_path equal to a fresh handle's at every step), and the polish
    workspace, its tables and the early-polish flags of one configuration must not leak into the next.  Every trajectory against the oracle."""
    seq = SMALL["C_" + kind]()
    snaps = check_sequence(seq, hip, oracle, monkeypatch.setenv)
    ok = [np.mean(s["stats"]["status"] == T.capi.SOLVE_SUCCEEDED) for s in snaps]
    assert min(ok[0], ok[1], ok[2], ok[4]) > 0.9, ok
    assert snaps[0]["stats"]["iterations_pn"].max() >= 1 and snaps[4]["stats"]["iterations_pn"].max() >= 1      # the polish ran, before and after


def test_sequence_D_replaced_descriptors(hip, oracle, monkeypatch):
    """to_set_cost on costs that carry per-trajectory terms (the terms start over) and to_set_constraint on a flagged GoalConstraint (shared
    parameters again) while the LinearConstraint keeps one right-hand side per trajectory, each followed by a solve."""
    seq = SMALL["D"]()
    snaps = check_sequence(seq, hip, oracle, monkeypatch.setenv)
    for s in snaps:
        assert (s["stats"]["status"] == T.capi.SOLVE_SUCCEEDED).all()
