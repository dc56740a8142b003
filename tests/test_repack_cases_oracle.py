"""Vets the cases of tests/test_gpu_repack_small.py (tests/repack_cases.py) on the CPU oracle alone, in the manner of
tests/test_constraint_limits_oracle.py, before the HIP library is held to them at B = 200:

  * every solve of every case ends with at least 8 distinct iteration counts, and the host loop of the HIP library (repack_cases.predicted_moves,
    a model of csrc/trajopt_hip.hip solve_impl with TRAJOPT_REPACK=1, TRAJOPT_REPACK_AT=0.9) would move the case's last solve — the one that reads
    per-trajectory duals where there are any — through at least three levels; over all cases there is a move to fewer than 64 trajectories,
    one to a count that is no multiple of 64, one to more than 64 at level >= 2 and one to at most 2 (the GPU's own trace is the authority:
    test_gpu_repack_small.py::test_moves_happen_at_the_edges);
  * for the cases compared with the oracle trajectory by trajectory (cartpole_cl, dint2_cl, cartpole_all: B single-trajectory problems, each with
    ITS limit, goal and target in its descriptors) the integers of both solves survive a nudge of +-1e-12 on the control guess and X / U move by
    less than 1e-6 — no trajectory within rounding of a decision boundary, so iterations and status can be compared bit for bit;
  * the same fleet solved with the SHARED nominal limit takes another number of iterations in more than a third of the trajectories (a
    library that left ``cl`` at its home index while the trajectory moved would be seen on integers);
  * the limits bind: after the second iLQR solve some control is within 1e-3 of its own limit in more than half of the trajectories.

What was tried.  An unconstrained double integrator (the issue's dint1_plain, and the hybrid model without constraints) is linear-quadratic:
iLQR takes the exact Newton step and EVERY trajectory ends after 3 iterations whatever its start, so nothing drains and nothing moves.  A
large initial regularisation does not help (Altro's schedule sets rho to 0 after the first accepted step: still 3 iterations, tried with
bp_reg_initial 0.3 .. 30 and factors 1.002 .. 1.01).  Both cases therefore carry their bounds (dint1_bound: model_params_fleet's dint1_con;
hybrid_bound: test_hybrid_dims.hybrid_problem(constrained=True)) and are solved by iLQR on the augmented Lagrangian at a fixed penalty: the
active set changes from iteration to iteration and the counts spread over 2 .. 66.  Cartpole start states moved towards the goal by
10^U(-2, 0) (seeds 3 and 4: the first tried) drain from the first batch step; the constrained Cartpoles keep configs.cartpole_x0 — the
second solve of their loop drains to single trajectories.  dint2_cl with constraint_limit_fleets' own start positions (+-0.2) ends within
9 iterations (one move): positions in +-3 are used.  Seeds of the limits: see SEEDS_TRIED."""
import numpy as np
import pytest

import trajopt_amd as T
import repack_cases as R

B = 200
AT, RP_MIN = 0.9, 1
SEEDS_TRIED = {"cartpole_cl": (51,), "cartpole_all": (52,), "dint2_cl": (62,)}      # the first seed tried passes in every case


def _rel(A, Rf):
    n = A.shape[0]
    return np.abs(A - Rf).reshape(n, -1).max(axis=1) / np.maximum(1.0, np.abs(Rf).reshape(n, -1).max(axis=1))


@pytest.fixture(scope="module")
def moves(oracle):
    return {name: [R.predicted_moves(s.stats["iterations"], B, AT, RP_MIN) for s in R.reference(name, B, oracle)] for name in R.CASES}


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_drains_unevenly_on_the_oracle(name, oracle, moves):
    snaps = R.reference(name, B, oracle)
    assert len(snaps) == (2 if R.CASES[name](oracle, B, only=0).recipe == "al_loop" else 1)
    for k, s in enumerate(snaps):
        it = s.stats["iterations"]
        print(f"\n{name} solve {k}: {len(set(it))} distinct iteration counts (max {it.max()}), statuses {np.unique(s.stats['status'])}, predicted moves {moves[name][k]}")
        assert len(set(it)) >= 8
        assert np.isfinite(s.X).all() and np.isfinite(s.U).all()
    last = moves[name][-1]
    assert len(last) >= 3, last                                         # level 3 is reached
    counts = [c for _, c in last]
    assert all(a > b for a, b in zip(counts, counts[1:]))


def test_predicted_moves_cover_the_edges(moves):
    every = [mv for per_case in moves.values() for solve in per_case for mv in solve]
    assert any(c < 64 for _, c in every)
    assert any(c % 64 for _, c in every)
    assert any(c > 64 and lvl >= 2 for lvl, c in every)
    assert any(c <= 2 for _, c in every)


def test_a_move_is_predicted_whenever_a_tenth_has_left(oracle):
    """predicted_moves against the rule it models: a solve in which fewer than 90 % of the trajectories are left after some batch step, while
    more than one is still iterating, must move."""
    for name in R.CASES:
        for s in R.reference(name, B, oracle):
            active = np.array(R.active_counts(s.stats["iterations"], R.CAP + 1))
            if ((active < AT * B) & (active > 1)).any():
                assert R.predicted_moves(s.stats["iterations"], B, AT, RP_MIN), name
    assert R.predicted_moves(np.full(B, 7), B, AT, RP_MIN) == []             # everybody ends together: nothing to move
    assert R.predicted_moves(np.r_[np.full(100, 3), np.full(100, 40)], B, AT, RP_MIN) == [(0, 100)]
    assert R.predicted_moves(np.r_[np.full(100, 3), np.full(100, 40)], B, AT, 0) == []


def _limit_gap(name, U, X):
    """[B]: the smallest distance of a control of trajectory b to one of ITS limits."""
    if name == "dint2_cl":
        v, up, dn, x0 = R.dint2_limits(B)
        return np.minimum(np.abs(up[:, None, :] - U), np.abs(U - dn[:, None, :])).min(axis=(1, 2))
    up, dn = R.cartpole_bounds(B, R.CARTPOLE_CL_SEED if name == "cartpole_cl" else R.CARTPOLE_ALL_SEED)
    u = U[:, :, 0]
    return np.minimum(np.abs(up[:, None] - u), np.abs(u - dn[:, None])).min(axis=1)


@pytest.mark.parametrize("name", R.ORACLE_COMPARED)
def test_oracle_compared_case(name, oracle):
    ref = R.reference(name, B, oracle)
    # integers and answers survive a nudge of the control guess
    for eps in (1e-12, -1e-12):
        nd = R.reference(name, B, oracle, nudge=eps)
        for k, (a, b) in enumerate(zip(ref, nd)):
            for key in ("iterations", "status"):
                moved = np.flatnonzero(a.stats[key] != b.stats[key])
                assert moved.size == 0, f"{name} solve {k}: trajectories {moved} change their {key} under a nudge of {eps}"
            own = np.maximum(_rel(b.X, a.X), _rel(b.U, a.U))
            print(f"\n{name} solve {k}, nudge {eps:+.0e}: the oracle's own answer moves by <= {own.max():.2e} (trajectory {own.argmax()})")
            assert own.max() < 1e-6
    # the shared limit gives other integers
    sh = R.reference(name, B, oracle, shared=True)
    changed = ref[-1].stats["iterations"] != sh[-1].stats["iterations"]
    print(f"{name}: iteration counts changed by the limits in {100 * changed.mean():.0f} % of the trajectories")
    assert changed.mean() > 1 / 3
    # the limits bind
    gap = _limit_gap(name, ref[-1].U, ref[-1].X)
    print(f"{name}: a control within 1e-3 of its own limit in {100 * (gap < 1e-3).mean():.0f} % of the trajectories")
    assert (gap < 1e-3).mean() > 0.5


def test_singles_are_the_batch_rows(oracle):
    """``only=b`` builds trajectory b of the batch: for a case without per-trajectory limits the stacked singles equal the oracle's batch bit
    for bit (so the singles of the limited cases differ from their batch by the limits alone)."""
    got = R.run_singles(R.CASES["cartpole_duals"], oracle, 12)
    want = R.run(R.CASES["cartpole_duals"](oracle, 12))
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.stats["iterations"], b.stats["iterations"])
        np.testing.assert_array_equal(a.X, b.X); np.testing.assert_array_equal(a.U, b.U)
