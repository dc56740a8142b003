"""Sequences of differently configured solves on ONE handle (batched MPC: goals per trajectory set and cleared, descriptors replaced, duals
written, iLQR after AL after ALTRO) — their definitions, shared with tests/test_gpu_handle_reuse.py, and the CPU side of the large ones.

A sequence is a problem builder and a list of steps; a step is a reconfiguration of the long-lived handle through the public verbs, the
same configuration described FROM SCRATCH for a newly built problem, and a solver with its options.  Builders and goals are indexed by
the GLOBAL trajectory number, so a sub-sample of a large batch is a problem of its own.

check_sequence below is the runner: one long-lived problem, every step against a newly built problem and against the oracle.

The GPU test holds every step of the 40 000- and 70 000-trajectory sequences (A, B) against the oracle on a fixed sample of 512
trajectories with hard asserts (integers exact, X / U / J to 1e-6).  That is only sound where the oracle's own solve does not amplify a
last-bit difference into another integer path, so the inputs are chosen HERE, on the oracle alone (the method of
tests/test_oracle_sensitivity.py): the whole sequence is run on the sample three times — start states as they are, moved by +1 ulp and by
-1 ulp — and every step must give identical iterations / status on all 512 trajectories and X, U, cost within 1e-6 on the converged ones.
The goal ranges and seeds below pass; the GPU test uses exactly these."""
import math

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs


class Step:
    """name; reconf(p, idx, ctx): public verbs on the long-lived handle; fresh(p, idx, ctx): the same configuration applied to a newly
    built problem (no history); solver class and options; rtol of the oracle comparison."""

    def __init__(self, name, reconf, fresh, solver, kw=None, rtol=1e-6):
        self.name, self.reconf, self.fresh, self.solver, self.kw, self.rtol = name, reconf, fresh, solver, dict(kw or {}), rtol


class Sequence:
    """B: the batch; build(lib, idx): a new problem holding the global trajectories idx; prepare(lib, idx) -> ctx handed to every step."""

    def __init__(self, name, B, build, steps, prepare=None, env=None):
        self.name, self.B, self.build, self.steps, self.prepare, self.env = name, B, build, steps, prepare or (lambda lib, idx: {}), dict(env or {})


def sample_indices(B, seed=12):
    """The trajectories the oracle solves of a large batch: the first 128, the last 64 and 320 seeded random ones in between (512, ascending)."""
    mid = np.random.default_rng(seed).choice(np.arange(128, B - 64), size=320, replace=False)
    return np.sort(np.concatenate([np.arange(128), mid, np.arange(B - 64, B)]))


def solve_step(p, step):
    """Every solve states ALL its options (defaults + the step's): nothing is inherited from the options an earlier solver left on the handle."""
    return step.solver(p, T.SolverOptions(lib=p._lib, **step.kw)).solve()


def start_state(p):
    """Everything a solve starts from that a reconfiguration does not describe: the nominal states and controls, the initial states, and the
    duals and penalty of every constraint (an iLQR solve reads them; AL and ALTRO solves start by resetting them, like Altro's reset!)."""
    return dict(X=T.states(p), U=T.controls(p), x0=p.x0.copy(), duals=[I.get_duals(p, i) for i in range(len(p.constraints))])


def upload_start_state(p, st, sel):
    """The recorded start state of the trajectories sel (positions in the recording) into a newly built problem."""
    p.set_initial_state(st["x0"][sel])
    T.initial_states(p, st["X"][sel])
    T.initial_controls(p, st["U"][sel])
    for i, (lam, mu) in enumerate(st["duals"]):
        I.set_duals(p, i, lam[sel], mu[sel])


def snapshot(s, p):
    return dict(stats={k: v.copy() for k, v in s.stats.items()}, X=T.states(p), U=T.controls(p), J=T.cost(p), batch_steps=int(s.batch_steps))


# ---- the sequences ------------------------------------------------------------------------------------------------------------------------
U_COLD = np.full(1, 0.01)      # the Cartpole's cold start (configs.cartpole_problem)


def cart_goals(B, seed, lo=-4.0, hi=-0.5):
    """One goal per trajectory of the GLOBAL batch: the pole upright, the cart at +-10^U(lo, hi) (tests/test_goal_batch.py cartpole_goals gives
    the uniform draw).  Magnitudes spread over decades on purpose: a warm-started re-solve then needs anything from one iteration to the
    whole budget, so the batch drains unevenly and the repacked working set moves several times in EVERY solve of a sequence."""
    from test_goal_batch import cartpole_goals
    Xf = cartpole_goals(B, seed=seed)
    u = Xf[:, 0].copy()
    Xf[:, 0] = np.sign(u) * 10.0 ** (lo + (hi - lo) * np.abs(u))
    return Xf


def _noop(p, idx, ctx):
    pass


def _cold(p):
    T.initial_controls(p, U_COLD)


def sequence_A(order):
    """Repacked working set, constrained Cartpole, MPC style: every solve starts from the solution of the one before it.  The table of carried
    arrays changes from solve to solve ([.., lam, mu] -> [.., gl, lam, mu] -> [.., lam, mu, cp]: the same NUMBER of arrays -> [.., gl, lam, mu, cp]
    -> [.., lam, mu]), in both orders of gl and cp.  The first solve starts from the controls of an earlier solve (a handle of its own) for
    start states that have moved since by +-10^U(-4, -0.5)."""
    B = 40000
    x0 = configs.cartpole_x0(B)
    x0_moved = x0.copy()
    x0_moved[:, 0] += cart_goals(B, 20)[:, 0]
    kw = dict(iterations=25)

    def build(lib, idx, x0=x0_moved):
        p = configs.cartpole_problem(batch=len(idx), N=41, tf=2.0, constrained=True, u_bnd=10.0, lib=lib)
        p.set_initial_state(x0[idx])
        return p

    def prepare(lib, idx):
        p = build(lib, idx, x0)
        if hasattr(lib, "max_threads"):
            from oracle_binding import set_threads
            set_threads(p, lib.max_threads())
        T.iLQRSolver(p, T.SolverOptions(lib=lib, iterations=80)).solve()
        return {"U": T.controls(p)}
    G = {k: cart_goals(B, s) for k, s in (("gl", 21), ("cp", 22), ("both", 23))}
    gl = lambda p, idx, ctx: T.set_goal_state(p, G["gl"][idx], constraint=False)
    cp = lambda p, idx, ctx: T.set_goal_state(p, G["cp"][idx], objective=False)
    both = lambda p, idx, ctx: T.set_goal_state(p, G["both"][idx])

    def then(f, dual_update=False):
        def reconf(p, idx, ctx):
            if dual_update:
                I.dual_update(p)                    # per-trajectory duals and penalties from here on (an iLQR solve never resets them)
            T.clear_goal_state_batch(p)
            f(p, idx, ctx)
        return reconf
    mid = {"gl": gl, "cp": cp}
    first, second = order.split("_")
    S = T.iLQRSolver
    return Sequence("A_" + order, B, build, [
        Step("shared", lambda p, idx, ctx: T.initial_controls(p, ctx["U"]), _noop, S, kw),
        Step(first, then(mid[first], dual_update=True), mid[first], S, kw),
        Step(second, then(mid[second]), mid[second], S, kw),
        Step("both", both, both, S, kw),
        Step("cleared", then(_noop), _noop, S, kw)], prepare=prepare, env={"TRAJOPT_REPACK": "2048"})


def sequence_B():
    """Repacked working set, unconstrained Cartpole, growing first move: most of the batch starts converged (small first move) -> cold start of
    the whole batch (large first move: the working sets must grow) -> goals per trajectory (the table gains gl) -> cleared."""
    B = 70000
    x0 = configs.cartpole_x0(B)
    kw = dict(iterations=B_ITERATIONS)
    Gl = cart_goals(B, 31, -1.0, 0.0)
    cold = np.random.default_rng(7).random(B) < 0.1

    def build(lib, idx):
        p = configs.cartpole_problem(batch=len(idx), N=41, tf=2.0, lib=lib)
        p.set_initial_state(x0[idx])
        return p

    def prepare(lib, idx):       # the controls of an earlier solve, from a handle of its own
        p = build(lib, idx)
        if hasattr(lib, "max_threads"):
            from oracle_binding import set_threads
            set_threads(p, lib.max_threads())
        # (tolerances well below the sequence's: at the default cost_tolerance a re-solve from these controls ends after ONE iteration for 96 %
        # of the trajectories — from the controls of a default solve it goes on improving for tens of iterations, and the first move is as large as ever)
        T.iLQRSolver(p, T.SolverOptions(lib=lib, iterations=300, cost_tolerance=1e-7, gradient_tolerance=1e-6)).solve()
        return {"U": T.controls(p)}

    def warm(p, idx, ctx):
        U = ctx["U"].copy()
        U[cold[idx]] = U_COLD
        T.initial_controls(p, U)
    gl = lambda p, idx, ctx: T.set_goal_state(p, Gl[idx])
    return Sequence("B", B, build, [
        Step("mostly_converged", warm, _noop, T.iLQRSolver, kw),
        Step("cold", lambda p, idx, ctx: _cold(p), _noop, T.iLQRSolver, kw),
        Step("gl", lambda p, idx, ctx: (gl(p, idx, ctx), _cold(p)), gl, T.iLQRSolver, kw),
        Step("cleared", lambda p, idx, ctx: (T.clear_goal_state_batch(p), _cold(p)), _noop, T.iLQRSolver, kw),
    ], prepare=prepare, env={"TRAJOPT_REPACK": "2048"})


def sequence_C(kind):
    """Kernel-variant switches at small batch: ALTRO, shared goal -> ALTRO, one goal per trajectory on costs and GoalConstraint (general forward
    variant, expansion variant 7) -> AL, goals on the costs only -> cleared, iLQR from the AL solution WITH its duals and penalties -> ALTRO again
    (default variants, polish workspace and tables left by the flagged configuration).  Cartpole on the cooperative path and on the lane path, the
    Quadrotor with the C5 constraint set; problems, goals and options of tests/test_goal_batch.py::test_per_trajectory_goal_constraints_on_gpu."""
    from test_goal_batch import cartpole_goals
    if kind == "quadrotor":
        B, env, akw = 24, {}, dict(n_steps=configs.C5_PN_STEPS)
        u0 = T.Quadrotor().hover_control()
        x0 = configs.quadrotor_x0(B)

        def build(lib, idx):
            p = configs.quadrotor_problem(batch=len(idx), N=61, tf=3.0, constrained=True, goal_inds=configs.C5_GOAL_INDS, lib=lib)
            assert np.array_equal(p.xf, _QUAD_XF)
            p.set_initial_state(x0[idx])
            return p

        def goals(seed, r=0.6):
            Xf = np.tile(_QUAD_XF, (B, 1))
            Xf[:, :3] += np.random.default_rng(seed).uniform(-r, r, (B, 3))
            return Xf
    else:
        B = 300 if kind == "cartpole_lane" else 70
        env = {"TRAJOPT_BACKWARD": "lane", "TRAJOPT_ACCEPT_ROLL_MIN": "1"} if kind == "cartpole_lane" else {}
        akw, u0 = {}, U_COLD
        x0 = configs.cartpole_x0(B)

        def build(lib, idx):
            p = configs.cartpole_problem(batch=len(idx), constrained=True, lib=lib)
            p.set_initial_state(x0[idx])
            return p

        def goals(seed):
            Xf = cartpole_goals(B, seed=seed)
            Xf[:, 0] *= 0.5
            return Xf
    G1, G2 = goals(3 if kind != "quadrotor" else 4), (goals(6) if kind != "quadrotor" else goals(C_QUAD_SEED2, C_QUAD_RANGE2))
    cold = lambda p: T.initial_controls(p, u0)
    both = lambda p, idx, ctx: T.set_goal_state(p, G1[idx])
    costs_only = lambda p, idx, ctx: T.set_goal_state(p, G2[idx], constraint=False)
    return Sequence("C_" + kind, B, build, [
        Step("altro_shared", _noop, _noop, T.ALTROSolver, akw),
        Step("altro_goals", lambda p, idx, ctx: (both(p, idx, ctx), cold(p)), both, T.ALTROSolver, akw),
        Step("al_cost_goals", lambda p, idx, ctx: (T.clear_goal_state_batch(p), costs_only(p, idx, ctx), cold(p)), costs_only, T.ALSolver,
             dict(constraint_tolerance=1e-4), rtol=1e-5),
        Step("ilqr_cleared", lambda p, idx, ctx: T.clear_goal_state_batch(p), _noop, T.iLQRSolver, {}),
        Step("altro_again", lambda p, idx, ctx: cold(p), _noop, T.ALTROSolver, akw)], env=env)


# The Quadrotor's goals on the COSTS ONLY pull against the GoalConstraint, which keeps the shared target.  With offsets of +-0.6 m (the range of the
# goals that move cost and constraint together) the AL solve creeps for up to 1000 iterations at the largest penalties and 1-7 of the 24 trajectories
# change their iteration count when the oracle's own start states move by one ulp (seeds 6..9; so does the iLQR step behind it): no hard assert can
# stand on that.  With +-0.1 m every trajectory converges (at most 194 iterations) and all integer paths survive +-1 ulp
# (test_small_sequence_is_insensitive_on_the_oracle below).
C_QUAD_SEED2 = 6
C_QUAD_RANGE2 = 0.1
_QUAD_XF = np.zeros(13)
_QUAD_XF[:3] = [2.0, 3.0, 1.0]
_QUAD_XF[3:7] = [math.cos(math.radians(135.0) / 2), 0.0, 0.0, math.sin(math.radians(135.0) / 2)]     # configs.quadrotor_problem's goal (sequence_C's builder checks it)


def sequence_D():
    """Replaced descriptors between solves (tests/test_goal_batch.py linear_problem: a LinearConstraint with one right-hand side per trajectory and
    a GoalConstraint): everything flagged -> the scalar set_goal_state on the costs only (to_set_cost on costs that carry per-trajectory terms: they
    start over, both constraints stay flagged) -> goals per trajectory on the costs again, then the scalar verb on the constraints only
    (to_set_constraint on the flagged GoalConstraint: shared parameters again, while the LinearConstraint stays flagged)."""
    from test_goal_batch import linear_problem, linear_rhs
    B = 40
    bv = linear_rhs(B)
    rng = np.random.default_rng(9)
    xf = np.array([1.0, 2.0, 0.0, 0.0])
    G1, G2 = np.tile(xf, (B, 1)), np.tile(xf, (B, 1))
    G1[:, :2] += rng.uniform(-0.3, 0.3, (B, 2))
    G2[:, :2] += rng.uniform(-0.3, 0.3, (B, 2))
    xf1, xf2 = np.array([0.9, 2.1, 0.0, 0.0]), np.array([1.1, 1.9, 0.0, 0.0])
    u0 = np.array([0.3, 0.5])

    def build(lib, idx):
        p, x0 = linear_problem(lib, B, bv)
        assert len(idx) == B              # (the start states of this builder are drawn for the whole batch)
        T.initial_controls(p, u0)
        return p
    cold = lambda p: T.initial_controls(p, u0)
    s0 = lambda p, idx, ctx: T.set_goal_state(p, G1[idx])

    def s1(p, idx, ctx):
        T.set_goal_state(p, xf1, constraint=False)

    def s1_fresh(p, idx, ctx):
        T.set_goal_state(p, G1[idx], objective=False)
        T.set_goal_state(p, xf1, constraint=False)

    def s2(p, idx, ctx):
        T.set_goal_state(p, G2[idx], constraint=False)
        T.set_goal_state(p, xf2, objective=False)

    def s2_fresh(p, idx, ctx):
        # per-trajectory linear terms are stored relative to the cost's shared descriptor (to_set_cost_linear_batch) and added to it: the shared
        # goal the costs were given before is part of the configuration (q_desc + (q_b - q_desc) rounds differently for another q_desc)
        T.set_goal_state(p, xf1, constraint=False)
        s2(p, idx, ctx)
    return Sequence("D", B, build, [
        Step("all_flagged", s0, s0, T.ALTROSolver),
        Step("costs_replaced", lambda p, idx, ctx: (s1(p, idx, ctx), cold(p)), s1_fresh, T.ALSolver, rtol=1e-5),
        Step("goal_constraint_replaced", lambda p, idx, ctx: (s2(p, idx, ctx), cold(p)), s2_fresh, T.ALTROSolver)])


SMALL = {"C_cartpole": lambda: sequence_C("cartpole"), "C_cartpole_lane": lambda: sequence_C("cartpole_lane"), "C_quadrotor": lambda: sequence_C("quadrotor"),
         "D": sequence_D}


# ---- one sequence on a long-lived handle, every step against a handle without history and against the oracle ----------------------------------
class _Sampled:
    """The sampled trajectories of a solved problem, in the shape assert_solve_parity reads: .stats / .total_iterations of a solver, and what
    T.states / T.controls ask of a problem."""

    def __init__(self, snap, sel):
        self.stats = {k: v[sel] for k, v in snap["stats"].items()}
        self.total_iterations = int(self.stats["iterations"].sum())
        self._X, self._U = np.ascontiguousarray(snap["X"][sel]), np.ascontiguousarray(snap["U"][sel])
        (self.B, self.N, self.n), self.m = self._X.shape, self._U.shape[2]

    _pd = staticmethod(lambda a: a)

    def _call(self, name, out):
        out[...] = {"get_states": self._X, "get_controls": self._U}[name]


def solver_path(p):
    import ctypes as C
    info = (C.c_int32 * 8)()
    p._call("solver_path", info)
    return list(info)


def assert_same_snapshot(a, b, what):
    from test_gpu_pipeline import _assert_same
    _assert_same((a["stats"], a["X"], a["U"]), (b["stats"], b["X"], b["U"]))
    np.testing.assert_array_equal(a["J"], b["J"], err_msg=what + ": cost")
    assert a["batch_steps"] == b["batch_steps"], (what, a["batch_steps"], b["batch_steps"])


def check_sequence(seq, lib, oracle, setenv, sample=None, fresh_env=None, guard=True, paths=True, per_step=None):
    """Runs seq on ONE long-lived problem of `lib`.  For every step: (1) the reconfiguration through the public verbs; (2) the complete start
    state of the solve is recorded — nominal states and controls, initial states, duals and penalty of every constraint (start_state); (3) the
    solve, and a snapshot of stats, X, U, cost, batch steps (and solver_path); (4) a NEWLY BUILT problem of `lib`, brought into the step's
    configuration from scratch, the recorded start state uploaded, the same solver and options: every output BIT-IDENTICAL (fresh_env: environment
    of that problem's creation, e.g. TRAJOPT_REPACK=0 — no working set at all); (5) a newly built ORACLE problem the same way — the whole batch, or
    the trajectories `sample` — held to assert_solve_parity (integers exact, step.rtol, 1e-4 on the trajectories cut off at an iteration limit).
    Then, with `guard`, the whole sequence once more under TRAJOPT_GUARD=1: every step equal to the unguarded one bit for bit.
    per_step(i, step, start, snap, p): the sequence's own asserts.  Returns the snapshots."""
    from oracle_binding import set_threads
    from test_gpu_parity import assert_solve_parity
    idx = np.arange(seq.B)
    sel = idx if sample is None else sample
    for k, v in seq.env.items():
        setenv(k, v)
    setenv("TRAJOPT_GUARD", "0")
    ctx = seq.prepare(lib, idx)
    p = seq.build(lib, idx)
    snaps = []
    for i, step in enumerate(seq.steps):
        what = f"{seq.name} step {i} ({step.name})"
        step.reconf(p, idx, ctx)
        start = start_state(p)
        s = solve_step(p, step)
        snap = snapshot(s, p)
        if paths:
            snap["path"] = solver_path(p)
        if per_step:
            per_step(i, step, start, snap, p)
        # a handle without history
        for k, v in (fresh_env or {}).items():
            setenv(k, v)
        f = seq.build(lib, idx)
        for k in (fresh_env or {}):
            setenv(k, seq.env[k])
        step.fresh(f, idx, ctx)
        upload_start_state(f, start, idx)
        want = snapshot(solve_step(f, step), f)
        assert_same_snapshot(snap, want, what + " against a fresh handle")
        if paths:
            mask = [0] * 7 + [2 if fresh_env else 0]       # (bit 1 of info[7] says "this handle repacks": the fresh one was created not to)
            assert [a & ~m for a, m in zip(snap["path"], mask)] == [a & ~m for a, m in zip(solver_path(f), mask)], what
        del f
        # the oracle
        o = seq.build(oracle, sel)
        set_threads(o, oracle.max_threads())
        step.fresh(o, sel, ctx)
        upload_start_state(o, start, sel)
        so = solve_step(o, step)
        if sample is None:
            assert_solve_parity(s, so, p, o, rtol=step.rtol, unconverged_rtol=1e-4)
        else:
            v = _Sampled(snap, sel)
            assert v.B == len(sel) == so.stats["iterations"].size      # no sampled trajectory is left out
            assert_solve_parity(v, so, v, o, rtol=step.rtol, unconverged_rtol=1e-4)
        del o
        snaps.append(snap)
    del p
    if guard:
        setenv("TRAJOPT_GUARD", "1")
        p = seq.build(lib, idx)
        for i, step in enumerate(seq.steps):
            step.reconf(p, idx, ctx)
            assert_same_snapshot(snaps[i], snapshot(solve_step(p, step), p), f"{seq.name} step {i} ({step.name}) under the guard")
        setenv("TRAJOPT_GUARD", "0")
    return snaps


B_ITERATIONS = 80     # as tests/test_gpu_parity.py::test_repacked_working_set

LARGE = {"A_gl_cp": lambda: sequence_A("gl_cp"), "A_cp_gl": lambda: sequence_A("cp_gl"), "B": sequence_B}


# ---- CPU: the oracle against itself on the sample ------------------------------------------------------------------------------------------
def _run_on_oracle(seq, oracle, idx, ulps):
    from oracle_binding import set_threads
    ctx = seq.prepare(oracle, idx)
    p = seq.build(oracle, idx)
    set_threads(p, oracle.max_threads())
    x0 = p.x0.copy()
    if ulps:
        moved = np.nextafter(x0, np.inf if ulps > 0 else -np.inf)
        p.set_initial_state(np.where(x0 != 0.0, moved, x0))          # (an exact zero stays: one ulp of zero is a denormal, not a rounding error)
    out = []
    for step in seq.steps:
        step.reconf(p, np.asarray(idx), ctx)
        out.append(snapshot(solve_step(p, step), p))
    return out


def check_oracle_sensitivity(name, oracle):
    from test_oracle_sensitivity import relerr
    if name in LARGE:
        seq = LARGE[name]()
        idx = sample_indices(seq.B)
        assert idx.size == 512 and np.unique(idx).size == 512
    else:
        seq = SMALL[name]()
        idx = np.arange(seq.B)
    base = _run_on_oracle(seq, oracle, idx, 0)
    for ulps in (+1, -1):
        moved = _run_on_oracle(seq, oracle, idx, ulps)
        for step, a, b in zip(seq.steps, base, moved):
            sa, sb = a["stats"], b["stats"]
            done = sa["status"] == T.capi.SOLVE_SUCCEEDED
            err = np.maximum.reduce([relerr(a["X"], b["X"]), relerr(a["U"], b["U"]), relerr(sa["cost"][:, None], sb["cost"][:, None])])
            print(f"{name} step {step.name} ({ulps:+d} ulp): iterations differ on {int((sa['iterations'] != sb['iterations']).sum())}, status on "
                  f"{int((sa['status'] != sb['status']).sum())} of {idx.size}; {int(done.sum())} converged, X/U/J on those within {err[done].max() if done.any() else 0.0:.2e}; "
                  f"{len(set(sa['iterations']))} distinct iteration counts")
            np.testing.assert_array_equal(sa["iterations"], sb["iterations"], err_msg=f"{name} {step.name} {ulps:+d} ulp")
            np.testing.assert_array_equal(sa["status"], sb["status"], err_msg=f"{name} {step.name} {ulps:+d} ulp")
            assert not done.any() or err[done].max() <= 1e-6, (name, step.name, ulps, err[done].max())


def test_sequence_A_gl_cp_sample_is_insensitive_on_the_oracle(oracle):
    check_oracle_sensitivity("A_gl_cp", oracle)


def test_sequence_A_cp_gl_sample_is_insensitive_on_the_oracle(oracle):
    check_oracle_sensitivity("A_cp_gl", oracle)


def test_sequence_B_sample_is_insensitive_on_the_oracle(oracle):
    check_oracle_sensitivity("B", oracle)


@pytest.mark.parametrize("name", ["C_cartpole", "C_quadrotor", "D"])
def test_small_sequence_is_insensitive_on_the_oracle(name, oracle):
    """The same for the small sequences, all trajectories (C on the lane path has the Cartpole problem of C_cartpole at another batch size)."""
    check_oracle_sensitivity(name, oracle)


@pytest.mark.parametrize("name", ["C_cartpole", "D"])
def test_small_sequences_on_the_oracle_alone(name, oracle, monkeypatch):
    """The sequence definitions themselves, on the CPU: the oracle as the long-lived handle against newly built oracle problems — every step
    bit-identical, so the "from scratch" description of every step IS the configuration its history of reconfigurations leaves, and the
    recorded start state is complete (the oracle keeps per-trajectory copies of the descriptors and no caches)."""
    check_sequence(SMALL[name](), oracle, oracle, monkeypatch.setenv, guard=False, paths=False)
