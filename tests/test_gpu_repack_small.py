"""The repacked working set (csrc/trajopt_hip.hip rp_setup / rp_move / rp_finish, csrc/k_generic.h k_repack_move / k_repack_home /
k_repack_list) at SMALL batch: TRAJOPT_BACKWARD=lane forces the fused lane kernel with compaction at any B, TRAJOPT_REPACK=1 lets a set of any
size move again, TRAJOPT_REPACK_AT=0.9 as soon as a tenth of it has finished — a batch of 200 moves again and again, down to single
trajectories, through both working sets and a composed map.  The large tests (test_gpu_parity.py::test_repacked_working_set,
test_gpu_pipeline.py::test_repacked_working_set_carries_duals, test_gpu_handle_reuse.py A / B) move tens of thousands of Cartpoles; here
every carried array (gl, lam, mu, cp, cl), every model of the fused lane path (Cartpole, double integrator D = 1 and D = 2 with m = 2, the
hybrid double integrator with its zero-padded knots) and the edges of the move (fewer than 64 trajectories, one, a count one past a tile,
three and more levels) are run, each in a second or so.  Cases: tests/repack_cases.py, vetted on the CPU by tests/test_repack_cases_oracle.py.

No getter reports the per-trajectory goal terms (gl) or GoalConstraint targets (cp); they are read back through what is computed from the HOME
arrays after the solve: T.cost (gl) and T.evaluate_constraints (x_N - cp_b), next to to_get_constraint_limits_batch for cl."""
import ctypes as C
import re

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import repack_cases as R
from test_handle_reuse_oracle import solver_path, start_state, upload_start_state

pytestmark = pytest.mark.gpu

AT = 0.9
BATCHES = [64, 65, 130, 200]


@pytest.fixture(autouse=True)
def lane_everywhere(monkeypatch):
    monkeypatch.setenv("TRAJOPT_BACKWARD", "lane")      # (every knob here is read when a handle is made)
    monkeypatch.setenv("TRAJOPT_REPACK_AT", str(AT))
    monkeypatch.setenv("TRAJOPT_GUARD", "0")
    monkeypatch.delenv("TRAJOPT_SYNC_DEBUG", raising=False)


def _same_bytes(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _same_snapshot(a, b, what):
    assert set(a.stats) == set(b.stats)
    for k in a.stats:
        _same_bytes(a.stats[k], b.stats[k], f"{what}: stat {k}")
    _same_bytes(a.X, b.X, what + ": states"); _same_bytes(a.U, b.U, what + ": controls"); _same_bytes(a.J, b.J, what + ": cost")
    assert a.batch_steps == b.batch_steps, what


def _drains_unevenly(snap, B, what, rp_min=1, at=AT):
    """tests/test_gpu_handle_reuse.py _drains_unevenly at this file's knobs: many distinct iteration counts, and at some batch step fewer than
    `at` of the batch was still iterating while more than rp_min were."""
    it = snap.stats["iterations"]
    active = np.array([(it > k).sum() for k in range(int(it.max()) + 1)])
    assert len(set(it)) > 10, (what, sorted(set(it)))
    assert ((active > rp_min) & (active < at * B)).any(), (what, active)


def _build(name, hip, B, setenv, repack):
    setenv("TRAJOPT_REPACK", repack)
    c = R.CASES[name](hip, B)
    path = solver_path(c.p)
    assert path[0] == 2 and path[1] == 1 and path[2] == 1, (name, "the fused lane path with compaction", path)
    assert bool(path[7] & 2) == (repack != "0"), (name, repack, path)
    return c


def _check_set_arrays(c, other, what):
    """What was set per trajectory is what the handle holds after the solve — the kind-3 arrays are never copied home, and the home pointers
    must be back — and what the never-moving handle `other` computes from its own."""
    p = c.p
    for con, lim in c.cl.items():
        _same_bytes(T.get_constraint_limits_batch(p, con), np.ascontiguousarray(lim), f"{what}: limits of constraint {con}")
    X = T.states(p)
    for con, par in c.cp.items():
        inds = [j - 1 for j in p.constraints.constraints[con].inds]
        vals = T.evaluate_constraints(p, con)
        _same_bytes(vals, T.evaluate_constraints(other.p, con), f"{what}: GoalConstraint values")
        np.testing.assert_array_equal(vals.reshape(p.B, -1), X[:, -1, inds] - par[:, inds], err_msg=f"{what}: x_N - cp_b")
    if c.gl is not None:
        _same_bytes(T.stage_costs(p), T.stage_costs(other.p), f"{what}: stage costs (goal terms)")
        assert np.ptp(c.gl[:, 0]) > 0


# ---- a. bit identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_repacked_solve_is_the_never_moving_solve(name, B, hip, monkeypatch):
    c1 = _build(name, hip, B, monkeypatch.setenv, "1")
    c0 = _build(name, hip, B, monkeypatch.setenv, "0")
    U0 = T.controls(c1.p)
    got, want = R.run(c1), R.run(c0)
    for k, (a, b) in enumerate(zip(got, want)):
        _same_snapshot(a, b, f"{name} B={B} solve {k}")
    _drains_unevenly(got[-1], B, f"{name} B={B}")
    _check_set_arrays(c1, c0, f"{name} B={B}")
    if c1.hybrid:
        nx, nu = c1.p.knot_dims()
        for k in range(c1.p.N):
            assert not got[-1].X[:, k, nx[k]:].any(), f"padded states of knot {k + 1}"
        for k in range(c1.p.N - 1):
            assert not got[-1].U[:, k, nu[k]:].any(), f"padded controls of step {k + 1}"
    # a second solve on the same handle starts from the home arrays again (from the first guess, with the duals the loop left: it drains again)
    again = []
    for c in (c1, c0):
        T.initial_controls(c.p, U0)
        s = T.iLQRSolver(c.p, T.SolverOptions(lib=hip, iterations=R.CAP, **c.kw)).solve()
        again.append(R.snapshot(s, c.p))
    _same_snapshot(again[0], again[1], f"{name} B={B} second solve on the handle")
    _drains_unevenly(again[0], B, f"{name} B={B} second solve on the handle")
    _check_set_arrays(c1, c0, f"{name} B={B} second solve on the handle")


# ---- b. the moves really happened, and at the edges --------------------------------------------------------------------------------------
MOVE = re.compile(r"\[sync-debug\] rp_move level (\d+) -> (\d+) count (\d+) \(B (\d+) Bp (\d+), cap (\d+) / (\d+)\) after k_repack_move: (.*)")
STEP = re.compile(r"\[sync-debug\] step (\d+) B=(\d+) Bp=(\d+) level=(\d+) [^:]*: (.*)")
_traces = {}


def _trace(name, hip, capfd, setenv):
    """The moves of every solve of the case's recipe at B = 200, read from the library's own trace (TRAJOPT_SYNC_DEBUG=1 is read per solve and
    written to the C library's stderr): -> per solve (moves [(level, count, B, Bp)], steps [(B, Bp, level)]).  Run once per session."""
    if name in _traces:
        return _traces[name]
    c = _build(name, hip, 200, setenv, "1")
    setenv("TRAJOPT_SYNC_DEBUG", "1")
    capfd.readouterr()
    out = []

    def after_solve(k, snap):
        err = capfd.readouterr().err
        moves = [tuple(int(v) for v in m.groups()[:5]) + (m.group(8),) for m in MOVE.finditer(err)]
        steps = [tuple(int(v) for v in m.groups()[:4]) + (m.group(5),) for m in STEP.finditer(err)]
        out.append((moves, steps, err, snap))
    R.run(c, after_solve)
    _traces[name] = out
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_moves_of_a_batch_of_200(name, hip, capfd, monkeypatch):
    """The last solve of every case (the one that reads per-trajectory duals where there are any) moves through three levels at least, to
    strictly fewer trajectories each time, each set padded to the next multiple of 64."""
    solves = _trace(name, hip, capfd, monkeypatch.setenv)
    for k, (moves, steps, err, snap) in enumerate(solves):
        print(f"\n{name} solve {k}:\n" + "\n".join(l for l in err.splitlines() if "k_repack_move" in l))
        assert steps and all(s[4] == "no error" for s in steps) and all(m[5] == "no error" for m in moves), err
        B_now, level = 200, 0
        for lvl, nxt, count, B_old, Bp_old, _ in moves:
            assert (lvl, nxt) == (level, level + 1) and B_old == B_now and Bp_old == (B_now + 63) // 64 * 64, (moves, steps)
            assert 1 <= count < B_old and count <= AT * B_old
            B_now, level = count, nxt
        # every batch step ran on the set the last move left: count trajectories, padded to whole tiles of 64
        sizes = {0: 200, **{m[1]: m[2] for m in moves}}
        for step, Bs, Bps, lvl, _ in steps:
            assert Bs == sizes[lvl] and Bps == (Bs + 63) // 64 * 64, (step, Bs, Bps, lvl)
    moves = solves[-1][0]
    assert len(moves) >= 3 and moves[-1][1] >= 3, moves
    # the oracle's iteration counts are the GPU's on these problems: what the CPU suite predicted is what happened
    it = solves[-1][3].stats["iterations"]
    assert [(m[0], m[2]) for m in moves] == R.predicted_moves(it, 200, AT, 1), "the host-loop model of repack_cases.predicted_moves"


def test_moves_happen_at_the_edges(hip, capfd, monkeypatch):
    every = [m for name in R.CASES for solve in _trace(name, hip, capfd, monkeypatch.setenv) for m in solve[0]]
    counts = [(m[0], m[2]) for m in every]
    assert any(c < 64 for _, c in counts), counts
    assert any(c % 64 for _, c in counts), counts
    assert any(c > 64 and lvl >= 2 for lvl, c in counts), counts
    assert any(c <= 2 for _, c in counts), counts
    assert any(c == 1 for _, c in counts), counts                            # a working set of exactly one trajectory


# ---- c. against the oracle ---------------------------------------------------------------------------------------------------------------
def _relerr(A, Rf):
    n = A.shape[0]
    return np.abs(A - Rf).reshape(n, -1).max(axis=1) / np.maximum(1.0, np.abs(Rf).reshape(n, -1).max(axis=1))


@pytest.mark.parametrize("name", R.ORACLE_COMPARED)
def test_repacked_limits_against_the_oracle(name, hip, oracle, monkeypatch):
    """B single-trajectory oracle problems, each with trajectory b's own limit, goal and target in its descriptors, run through the same
    recipe.  Integers bit for bit, X / U / J to 1e-6 in the per-trajectory max norm (assert_solve_parity's measure).  The same fleet with the
    SHARED nominal limit takes other iteration counts in more than a third of the trajectories: a library that left cl behind at the home
    index while the trajectory moved fails here on integers."""
    B = 200
    ref = R.reference(name, B, oracle)
    shared = R.reference(name, B, oracle, shared=True)
    assert (ref[-1].stats["iterations"] != shared[-1].stats["iterations"]).mean() > 1 / 3
    c = _build(name, hip, B, monkeypatch.setenv, "1")
    got = R.run(c)
    _drains_unevenly(got[-1], B, name)
    for k, (a, b) in enumerate(zip(got, ref)):
        err = np.maximum.reduce([_relerr(a.X, b.X), _relerr(a.U, b.U), _relerr(a.J[:, None], b.J[:, None]),
                                 _relerr(a.stats["cost"][:, None], b.stats["cost"][:, None])])
        print(f"\n{name} solve {k}: iterations differ on {int((a.stats['iterations'] != b.stats['iterations']).sum())} of {B}, X / U / J within {err.max():.2e}")
        for key in ("iterations", "status"):
            np.testing.assert_array_equal(a.stats[key], b.stats[key], err_msg=f"{name} solve {k}: {key}")
        assert err.max() <= 1e-6, (name, k, err.argmax(), err.max())
    ls, J_next = R.ls_after(c.p)                                             # the line search the solve would run next, on the home arrays
    np.testing.assert_array_equal(ls, ref[-1].ls, err_msg=f"{name}: ls_index")
    assert _relerr(J_next[:, None], ref[-1].J_next[:, None]).max() <= 1e-6


# ---- d. k_accept_roll next to a small working set, under the guard ---------------------------------------------------------------------------
@pytest.mark.parametrize("fwd2", [None, "0"])
@pytest.mark.parametrize("name", ["cartpole_plain", "cartpole_cl"])
def test_accept_roll_next_to_a_small_working_set_under_the_guard(name, fwd2, hip, monkeypatch):
    """The shape of the overrun behind a working set: k_accept_roll's lanes without an accepted step store into the spare tile behind the set
    — at B = 130 a working set of 64 + 64 lanes is half spare tile.  Candidate controls only on every batch step (TRAJOPT_ACCEPT_ROLL_MIN=1,
    TRAJOPT_ACCEPT_ROLL_FRAC=0), every array between red zones: the solve ends clean and equals the unguarded solve that never moves.
    With the default TRAJOPT_FWD2 a batch this small runs two-wave workgroups, which store whole candidates, and k_accept_roll stays idle;
    TRAJOPT_FWD2=0 is what makes it run here (tests/test_gpu_parity.py::test_accept_by_rollout_small_models)."""
    B = 130
    monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_MIN", "1")
    monkeypatch.setenv("TRAJOPT_ACCEPT_ROLL_FRAC", "0")
    if fwd2 is not None:
        monkeypatch.setenv("TRAJOPT_FWD2", fwd2)
    monkeypatch.setenv("TRAJOPT_GUARD", "1")
    c1 = _build(name, hip, B, monkeypatch.setenv, "1")
    monkeypatch.setenv("TRAJOPT_GUARD", "0")
    c0 = _build(name, hip, B, monkeypatch.setenv, "0")
    assert solver_path(c1.p)[6] == 1 and solver_path(c0.p)[6] == 1
    got, want = R.run(c1), R.run(c0)                 # (a red zone written to ends the solve with a HipError that names the array and the step)
    for k, (a, b) in enumerate(zip(got, want)):
        _same_snapshot(a, b, f"{name} solve {k} under the guard")
    _drains_unevenly(got[-1], B, name)
    _check_set_arrays(c1, c0, name)


# ---- e. the table of carried arrays changes between solves, on one handle ------------------------------------------------------------------
def test_table_changes_between_solves_on_one_handle(hip, monkeypatch):
    """Shared bound -> set_bounds_batch (the table gains cl) -> set_goal_state on the costs (gains gl) -> limits cleared -> goals cleared, each
    followed by a repacked iLQR solve from a recorded start (cold controls; the duals of one update behind the first solve).  Every solve
    equals, byte for byte, the solve of a handle created with TRAJOPT_REPACK=0, configured from scratch and given the recorded start."""
    B = 200
    up, dn = R.cartpole_bounds(B, R.CARTPOLE_CL_SEED)
    Xf = R.cartpole_goals(B)
    limits = lambda p: T.set_bounds_batch(p, 0, u_max=up[:, None], u_min=dn[:, None])
    goals = lambda p: T.set_goal_state(p, Xf, constraint=False)
    steps = [("shared", lambda p: None, []),
             ("limits", limits, [limits]),
             ("limits and goals", goals, [limits, goals]),
             ("goals", T.clear_constraint_limits_batch, [goals]),
             ("cleared", T.clear_goal_state_batch, [])]
    p = _build("cartpole_duals", hip, B, monkeypatch.setenv, "1").p
    U0 = T.controls(p)
    solve = lambda q: R.snapshot(T.iLQRSolver(q, T.SolverOptions(lib=hip, iterations=R.CAP)).solve(), q)
    for i, (what, reconf, fresh) in enumerate(steps):
        reconf(p)
        T.initial_controls(p, U0)
        start = start_state(p)
        got = solve(p)
        f = _build("cartpole_duals", hip, B, monkeypatch.setenv, "0").p
        for fn in fresh:
            fn(f)
        upload_start_state(f, start, np.arange(B))
        _same_snapshot(got, solve(f), f"step {i} ({what}) against a fresh handle that never moves")
        _drains_unevenly(got, B, what)
        want_limits = np.stack([up, dn], axis=1) if limits in fresh else np.tile([R.U_NOMINAL, -R.U_NOMINAL], (B, 1))
        _same_bytes(T.get_constraint_limits_batch(p, 0), want_limits, f"step {i} ({what}): limits")
        if i == 0:
            I.dual_update(p)                         # per-trajectory duals and penalties from here on (an iLQR solve never resets them)
            lam = I.get_duals(p, 0)[0]
            assert np.ptp(np.abs(lam).reshape(B, -1).max(axis=1)) > 0


# ---- f. who must not repack ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plants", "time_steps"])
def test_handles_that_must_not_repack(kind, hip, capfd, monkeypatch):
    """One plant or one set of time steps per trajectory: such a handle addresses the batch by position and never moves it, whatever the knobs
    say — no repack bit in solver_path, no rp_move in the trace, the bits of the TRAJOPT_REPACK=0 solve."""
    import model_params_fleet as M
    import time_step_fleets as S
    B = 200

    def build(repack):
        monkeypatch.setenv("TRAJOPT_REPACK", repack)
        c = R.CASES["cartpole_plain"](hip, B)
        if kind == "plants":
            T.set_model_params(c.p, M.draw_models("cartpole", B, 71))
        else:
            T.set_time_steps_batch(c.p, S.draw_steps(R.TF, R.N, B, 72, ragged=True))
        return c
    c1, c0 = build("1"), build("0")
    assert solver_path(c1.p)[7] & 2 == 0 and solver_path(c0.p)[7] & 2 == 0
    monkeypatch.setenv("TRAJOPT_SYNC_DEBUG", "1")
    capfd.readouterr()
    got = R.run(c1)
    err = capfd.readouterr().err
    monkeypatch.delenv("TRAJOPT_SYNC_DEBUG")
    assert "[sync-debug] step" in err and "rp_move" not in err
    want = R.run(c0)
    _same_snapshot(got[0], want[0], kind)
    assert len(set(got[0].stats["iterations"])) > 10
