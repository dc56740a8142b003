"""The batches of tests/failure_cases.py — trajectories that restart their backward pass at different regularisation levels, run
into bp_reg_max, fail their line search, end MAXIMUM_COST / NO_PROGRESS / REGULARIZATION_MAX, several classes inside one wave — on
every kernel path, against the CPU oracle.  tests/test_failure_cases_oracle.py vets the inputs on the oracle alone (populated
classes, decision margins, integers stable under last-bit changes of the inputs, value mask); this file holds the kernels to them:
single phases, short solves, the bit identities between kernel paths, and one NaN pivot.

Trip count of the restart loops (read in k_backward.h k_backward_coop / k_backward_lane / k_backward_mfma, k_expand.h
k_expand_backward_lane / k_expand_backward_coop, k_scan.h k_expand_backward_scan before any of this ran): every copy restarts only after
reg_increase (common.h) and only while rho <= bp_reg_max; reg_increase sets drho = max(drho f, f) >= f and rho = max(rho drho, bp_reg_min),
so from the second failure on rho grows by a factor >= f = bp_reg_increase_factor per restart, whatever the pivot was (a NaN pivot fails
the test `!(s > 0)` / not_positive like a negative one and feeds nothing into rho).  Restarts per pass <= 1 + log(bp_reg_max / bp_reg_min)
/ log(f): 80 with the defaults (1e8, 1e-8, 1.6) — 13 in fact, since drho grows as well — each of at most N - 1 knots.  The scan kernel adds
one pass (its scan attempt) in front.  No input of this file can make a kernel spin."""
import ctypes

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import failure_cases as F

pytestmark = pytest.mark.gpu
S = T.capi

# knobs (read when a handle is created) -> what to_solver_path must report: (info[0] backward flavour, info[1] fused, info[5] scan[,
# info[4] waves per forward-pass workgroup: 1 = k_forward, 2 = k_forward2]); None: not asserted
PHASE_PATHS = {
    "coop": ({"TRAJOPT_BACKWARD": "coop", "TRAJOPT_SCAN": "0"}, (0, None, 0)),     # k_backward_coop
    "lane": ({"TRAJOPT_BACKWARD": "lane"}, (2, None, 0)),                            # k_backward_lane
    "mfma": ({"TRAJOPT_BACKWARD": "mfma"}, (1, 0, 0)),                               # k_backward_mfma
    "scan": ({"TRAJOPT_BACKWARD": "coop", "TRAJOPT_SCAN": "2"}, (0, 1, 1)),         # k_expand_backward_scan (phase API: TRAJOPT_SCAN=2)
}
SOLVE_PATHS = {
    "default": ({}, None),
    "fused_coop": ({"TRAJOPT_BACKWARD": "coop", "TRAJOPT_SCAN": "0"}, (0, 1, 0)),                             # k_expand_backward_coop
    "split_coop": ({"TRAJOPT_BACKWARD": "coop", "TRAJOPT_SCAN": "0", "TRAJOPT_FUSED_COOP": "0"}, (0, 0, 0)),  # k_expand + k_backward_coop
    "scan": ({"TRAJOPT_BACKWARD": "coop", "TRAJOPT_SCAN": "1"}, (0, 1, 1)),                                   # k_expand_backward_scan
    "fused_lane": ({"TRAJOPT_BACKWARD": "lane"}, (2, 1, 0)),                                                  # k_expand_backward_lane
    "split_lane": ({"TRAJOPT_BACKWARD": "lane", "TRAJOPT_FUSED_LANE": "0"}, (2, 0, 0)),                       # k_expand_lane + k_backward_lane
    "mfma": ({"TRAJOPT_BACKWARD": "mfma"}, (1, 0, 0)),                                                        # k_backward_mfma
    "fwd1": ({"TRAJOPT_FWD2": "0"}, (None, None, None, 1)),                                                   # k_forward
    "fwd2": ({"TRAJOPT_FWD2": "1"}, (None, None, None, 2)),                                                   # k_forward2
}
UNCONSTRAINED_SMALL = ["cartpole_levels", "cartpole_regmax", "cartpole_max_cost", "cartpole_no_progress", "di2_uniform"]
CONSTRAINED_SMALL = ["cartpole_al", "di2_levels", "di2_regmax", "di2_altro"]
QUADROTOR = ["quadrotor_w10", "quadrotor_w7", "quadrotor_regmax"]


def solver_path(p):
    info = (ctypes.c_int32 * 8)()
    p._call("solver_path", info)
    return list(info)


def assert_path(p, want, what):
    info = solver_path(p)
    if want is not None:
        for i, w in zip((0, 1, 5, 4), want):
            assert w is None or info[i] == w, f"{what}: to_solver_path reports {info}, wanted info[{i}] == {w}"
    return info


def with_env(monkeypatch, env, f):
    with monkeypatch.context() as mp:
        for k in ("TRAJOPT_BACKWARD", "TRAJOPT_SCAN", "TRAJOPT_FUSED_COOP", "TRAJOPT_FUSED_LANE", "TRAJOPT_FWD2", "TRAJOPT_COMPACT"):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        return f()


_oracle = {}


def oracle_first_pass(name, oracle):
    if ("first", name) not in _oracle:
        _oracle[("first", name)] = F.CASES[name].first_pass(oracle)
    return _oracle[("first", name)]


def oracle_solve(name, oracle):
    if ("solve", name) not in _oracle:
        _oracle[("solve", name)] = F.CASES[name].solve(oracle)[:3]
    return _oracle[("solve", name)]


# ------------------------------------------------------------------------------------------------------------- 2. single phases
# (the 2-D double integrator has no MFMA backward pass compiled: TRAJOPT_BACKWARD=mfma leaves it on the cooperative kernel)
PHASE_CASES = ([(n, p) for n in UNCONSTRAINED_SMALL for p in ("coop", "lane", "mfma", "scan") if p != "mfma" or not n.startswith("di2")]
               + [(n, p) for n in CONSTRAINED_SMALL[:3] for p in ("coop", "lane", "mfma") if p != "mfma" or not n.startswith("di2")]
               + [(n, "default") for n in QUADROTOR])


@pytest.mark.parametrize("name,path", PHASE_CASES)
def test_one_iteration_phase_by_phase(name, path, hip, oracle, monkeypatch):
    """rollout / expand / backwardpass / gains / forwardpass from identical inputs, on the backward kernel the knobs select (asserted
    with to_solver_path), against the oracle: rho bit for bit (after the backward pass AND after the forward pass, where a failed
    search has raised it), K / d at rtol 1e-7 / atol 1e-9 and dV at rtol 1e-8 (the tolerances of test_backward_and_forward, kept
    meaningful by the decision margins the CPU test asserts), line-search index equal, J at 1e-8; a trajectory whose backward pass ran
    into bp_reg_max reports rho > bp_reg_max, a failed search (-1), J unchanged and keeps its trajectory to the last bit."""
    case = F.CASES[name]
    env, want = PHASE_PATHS.get(path, ({}, (1, 0, 0)))     # the Quadrotor's default is the MFMA kernel

    def run():
        p = case.build(hip)
        assert_path(p, want, f"{name} on {path}")
        T.rollout(p)
        X0, U0 = T.states(p), T.controls(p)
        J0 = I.al_cost(p)
        I.expand(p); I.backwardpass(p)
        g = I.gains(p)
        ls, J = I.forwardpass(p)
        return g, ls, J, T.states(p), T.controls(p), I.gains(p)["rho"], X0, U0, J0
    g, ls, J, X, U, rho_after, X0, U0, J0 = with_env(monkeypatch, env, run)
    o = oracle_first_pass(name, oracle)
    go = o["gains"]
    np.testing.assert_array_equal(g["rho"], go["rho"])
    fail = o["bpfail"]
    ok = ~fail
    print(f"\n{name} on {path}: rho levels {dict(zip(*np.unique(np.round(go['rho'], 6), return_counts=True)))}, {int(fail.sum())} failed passes, "
          f"{int((o['ls'] < 0).sum() - fail.sum())} failed searches")
    np.testing.assert_allclose(g["K"][ok], go["K"][ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["d"][ok], go["d"][ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["dV"][ok], go["dV"][ok], rtol=1e-8)
    np.testing.assert_array_equal(ls, o["ls"])
    np.testing.assert_allclose(J, o["J"], rtol=1e-8)
    np.testing.assert_array_equal(rho_after, o["rho_after"])
    np.testing.assert_allclose(X, o["X"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(U, o["U"], rtol=1e-7, atol=1e-9)
    # no step for a failed pass
    assert (ls[fail] == -1).all()
    np.testing.assert_array_equal(J[fail], J0[fail])
    np.testing.assert_array_equal(X[fail], X0[fail]); np.testing.assert_array_equal(U[fail], U0[fail])
    np.testing.assert_array_equal(rho_after[fail], g["rho"][fail])
    # a failed search keeps the nominal as well
    lsf = (ls < 0) & ok
    np.testing.assert_array_equal(X[lsf], X0[lsf]); np.testing.assert_array_equal(U[lsf], U0[lsf])


@pytest.mark.parametrize("pair,path", [(("cartpole_levels", "cartpole_regmax"), p) for p in ("coop", "lane", "mfma", "scan")]
                         + [(("di2_levels", "di2_regmax"), p) for p in ("coop", "lane")]
                         + [(("quadrotor_w10", "quadrotor_regmax"), "default")])
def test_failed_passes_leave_their_neighbours_alone(pair, path, hip, monkeypatch):
    """The same batch with bp_reg_max large (every trajectory finds its level) and with bp_reg_max below the top level (those fail,
    in the middle of their tiles / groups): the trajectories that do not fail have the SAME gains, dV and rho, bit for bit."""
    env, want = PHASE_PATHS.get(path, ({}, (1, 0, 0)))
    out = []
    for name in pair:
        def run():
            p = F.CASES[name].build(hip)
            assert_path(p, want, f"{name} on {path}")
            T.rollout(p); I.expand(p); I.backwardpass(p)
            return I.gains(p), p.case_options.bp_reg_max
        out.append(with_env(monkeypatch, env, run))
    (g0, _), (g1, rmax) = out
    fail = g1["rho"] > rmax
    assert 3 <= fail.sum() <= fail.size - 3
    for k in ("K", "d", "dV", "rho"):
        np.testing.assert_array_equal(g1[k][~fail], g0[k][~fail], err_msg=k)


@pytest.mark.parametrize("name,path", [(n, p) for n in ("cartpole_levels", "cartpole_regmax") for p in ("fused_lane", "fused_coop")]
                         + [(n, p) for n in ("cartpole_al", "di2_regmax") for p in ("fused_lane", "fused_coop")])
def test_first_pass_of_the_fused_kernels(name, path, hip, oracle, monkeypatch):
    """k_expand_backward_lane and k_expand_backward_coop run inside solves only: a solve cut off after ONE iteration leaves the gains,
    rho and dV of its first backward pass behind — against the oracle's after the same solve, restarts and failed passes included."""
    case = F.CASES[name]
    env, want = SOLVE_PATHS[path]
    res = {}
    for lib, key in ((hip, "hip"), (oracle, "oracle")):
        def run():
            p = case.build(lib, iterations=1, iterations_outer=1)
            if lib is hip:
                assert_path(p, want, f"{name} on {path}")
            s = (T.ALSolver if case.solver != "ilqr" else T.iLQRSolver)(p).solve()
            return I.gains(p), {k: np.array(v).copy() for k, v in s.stats.items()}, p.case_options.bp_reg_max
        res[key] = with_env(monkeypatch, env if lib is hip else {}, run)
    (g, st, rmax), (go, sto, _) = res["hip"], res["oracle"]
    for k in ("status", "iterations", "iterations_outer"):
        np.testing.assert_array_equal(st[k], sto[k], err_msg=k)
    # (a failed search has raised rho after the pass on both sides alike)
    np.testing.assert_array_equal(g["rho"], go["rho"])
    ok = ~(sto["status"] == S.REGULARIZATION_MAX)
    assert len(np.unique(go["rho"])) >= 3
    np.testing.assert_allclose(g["K"][ok], go["K"][ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["d"][ok], go["d"][ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["dV"][ok], go["dV"][ok], rtol=1e-8)


# -------------------------------------------------------------------------------------------------------------- 3. short solves
SOLVE_CASES = ([(n, p) for n in UNCONSTRAINED_SMALL for p in SOLVE_PATHS if p != "mfma" or not n.startswith("di2")]
               + [(n, p) for n in CONSTRAINED_SMALL for p in SOLVE_PATHS if p != "scan" and (p != "mfma" or not n.startswith("di2"))]
               + [(n, p) for n in QUADROTOR for p in ("default", "fwd1", "fwd2")])


def assert_case_solve(name, st, X, U, oracle):
    """Integers equal to the oracle's for every trajectory; X, U, cost at 1e-6 on the trajectories of the value mask; the status
    histogram the case was built for."""
    case = F.CASES[name]
    sto, Xo, Uo = oracle_solve(name, oracle)
    for k in ("status", "iterations", "iterations_outer", "iterations_pn"):
        np.testing.assert_array_equal(st[k], sto[k], err_msg=k)
    assert st["total_iterations"] == sto["total_iterations"]
    hist = dict(zip(*np.unique(sto["status"], return_counts=True)))
    for s in case.statuses:
        assert (st["status"] == s).sum() == hist.get(s, 0) >= 1, f"status {s}: {hist}"
    m = F.value_mask(case, oracle)
    ex, eu = F.trajectory_error(X, Xo), F.trajectory_error(U, Uo)
    print(f"\n{name}: largest error on the {int(m.sum())} masked trajectories X {ex[m].max():.2e} U {eu[m].max():.2e}, "
          f"on the {int((~m).sum())} others X {ex[~m].max(initial=0):.2e} U {eu[~m].max(initial=0):.2e}")
    assert F.trajectories_close(X, Xo, 1e-6)[m].all(), f"X: trajectories {np.where(~F.trajectories_close(X, Xo, 1e-6) & m)[0]}"
    assert F.trajectories_close(U, Uo, 1e-6)[m].all(), f"U: trajectories {np.where(~F.trajectories_close(U, Uo, 1e-6) & m)[0]}"
    np.testing.assert_allclose(st["cost"][m], sto["cost"][m], rtol=1e-6)
    return hist


@pytest.mark.parametrize("name,path", SOLVE_CASES)
def test_short_solves(name, path, hip, oracle, monkeypatch):
    """The cases as iLQR / AL / ALTRO solves on every solve-loop path, against the oracle.  On the fused lane path this covers a
    backward pass that runs into bp_reg_max right AFTER an accepted step (cartpole_regmax, di2_regmax): k_expand_backward_lane
    writes the accepted step through to the nominal knot by knot as it expands, and has to finish that copy when it abandons the
    pass, or the trajectory ends as half the old and half the new one with every integer still equal."""
    env, want = SOLVE_PATHS[path]
    case = F.CASES[name]

    def run():
        st, X, U, p = case.solve(hip)
        # (the Quadrotor keeps its default backward kernel: only the forward kernel of its rows is asserted)
        assert_path(p, want if case.small or path in ("fwd1", "fwd2") else None, f"{name} on {path}")
        return st, X, U
    st, X, U = with_env(monkeypatch, env, run)
    hist = assert_case_solve(name, st, X, U, oracle)
    print(f"\n{name} on {path}: statuses {hist}")
    if case.solver == "altro":
        # the polish takes exactly the trajectories the oracle's takes: those the AL stage left SOLVE_SUCCEEDED above the tolerance
        sto = oracle_solve(name, oracle)[0]
        failed = np.isin(sto["status"], (S.MAXIMUM_COST, S.MAX_ITERATIONS_OUTER, S.REGULARIZATION_MAX))
        assert failed.sum() >= 3 and (st["iterations_pn"][failed] == 0).all() and (st["iterations_pn"][~failed] >= 1).any()
        np.testing.assert_allclose(st["c_max"], sto["c_max"], rtol=1e-3, atol=1e-9)


def test_every_failure_status_is_exercised():
    """5, 8 and 10 each belong to a case of test_short_solves (which asserts their counts against the oracle's)."""
    covered = set(s for n in UNCONSTRAINED_SMALL + CONSTRAINED_SMALL + QUADROTOR for s in F.CASES[n].statuses)
    assert {S.MAXIMUM_COST, S.NO_PROGRESS, S.REGULARIZATION_MAX} <= covered


# ---------------------------------------------------------------------------------------------- 4. bit identities on failing batches
def solve_all(case, hip):
    st, X, U, p = case.solve(hip)
    return st, X, U, solver_path(p)


IDENTITIES = [
    # (what, case, common knobs, knob that must not change anything, its two values)
    ("compaction, fused lane", "cartpole_regmax", {"TRAJOPT_BACKWARD": "lane"}, "TRAJOPT_COMPACT", ("1", "0")),
    ("compaction, fused lane", "cartpole_no_progress", {"TRAJOPT_BACKWARD": "lane"}, "TRAJOPT_COMPACT", ("1", "0")),
    ("compaction, fused lane, AL", "cartpole_al", {"TRAJOPT_BACKWARD": "lane"}, "TRAJOPT_COMPACT", ("1", "0")),
    ("compaction, MFMA", "quadrotor_regmax", {}, "TRAJOPT_COMPACT", ("1", "0")),
    ("compaction, MFMA, small model, AL", "cartpole_al", {"TRAJOPT_BACKWARD": "mfma"}, "TRAJOPT_COMPACT", ("1", "0")),
    ("k_forward / k_forward2", "cartpole_regmax", {}, "TRAJOPT_FWD2", ("0", "1")),
    ("k_forward / k_forward2", "cartpole_no_progress", {}, "TRAJOPT_FWD2", ("0", "1")),
    ("k_forward / k_forward2", "cartpole_max_cost", {"TRAJOPT_BACKWARD": "lane"}, "TRAJOPT_FWD2", ("0", "1")),
    ("k_forward / k_forward2, AL", "cartpole_al", {}, "TRAJOPT_FWD2", ("0", "1")),
    ("k_forward / k_forward2", "quadrotor_regmax", {}, "TRAJOPT_FWD2", ("0", "1")),
    ("repacked last line-search round", "quadrotor_regmax", {"TRAJOPT_LS_DEEP": "0", "TRAJOPT_LS_CANDIDATES": "4"}, "TRAJOPT_LS_REPACK", ("0", "1")),
    ("repacked last line-search round, two waves", "quadrotor_w7", {"TRAJOPT_LS_DEEP": "0", "TRAJOPT_LS_CANDIDATES": "2", "TRAJOPT_FWD2": "1"}, "TRAJOPT_LS_REPACK", ("0", "1")),
    ("accept by rollout", "cartpole_regmax", {"TRAJOPT_FWD2": "0"}, "TRAJOPT_ACCEPT_ROLL_MIN", ("0", "1")),
    ("accept by rollout, fused lane", "cartpole_no_progress", {"TRAJOPT_FWD2": "0", "TRAJOPT_BACKWARD": "lane"}, "TRAJOPT_ACCEPT_ROLL_MIN", ("0", "1")),
    ("accept by rollout, fused lane", "cartpole_max_cost", {"TRAJOPT_FWD2": "0", "TRAJOPT_BACKWARD": "lane"}, "TRAJOPT_ACCEPT_ROLL_MIN", ("0", "1")),
    ("accept by rollout, AL", "cartpole_al", {"TRAJOPT_FWD2": "0"}, "TRAJOPT_ACCEPT_ROLL_MIN", ("0", "1")),
    ("accept by rollout, MFMA", "quadrotor_regmax", {"TRAJOPT_FWD2": "0"}, "TRAJOPT_ACCEPT_ROLL_MIN", ("0", "1")),
]
EXTRA_KNOBS = ("TRAJOPT_LS_DEEP", "TRAJOPT_LS_CANDIDATES", "TRAJOPT_LS_REPACK", "TRAJOPT_ACCEPT_ROLL_MIN", "TRAJOPT_REPACK", "TRAJOPT_REPACK_AT")


WORKING_SET = [
    ("repacked working set", "cartpole_regmax", {"TRAJOPT_BACKWARD": "lane", "TRAJOPT_REPACK_AT": "0.9"}, "TRAJOPT_REPACK", ("0", "8")),
    ("repacked working set", "cartpole_no_progress", {"TRAJOPT_BACKWARD": "lane", "TRAJOPT_REPACK_AT": "0.9"}, "TRAJOPT_REPACK", ("0", "8")),
    ("repacked working set", "cartpole_max_cost", {"TRAJOPT_BACKWARD": "lane", "TRAJOPT_REPACK_AT": "0.7"}, "TRAJOPT_REPACK", ("0", "8")),
]


def _ids(rows):
    return [f"{i[0]}-{i[1]}".replace(" ", "_").replace(",", "") for i in rows]


@pytest.mark.parametrize("what,name,common,knob,values", IDENTITIES, ids=_ids(IDENTITIES))
def test_kernel_choices_are_invisible_on_failing_batches(what, name, common, knob, values, hip, oracle, monkeypatch):
    """Where the suite asserts bit identity between two kernel paths on healthy batches, the same on a failing one: which lane or
    wave owns a trajectory, which forward kernel runs, how the line search is laid out and how the accepted step reaches the
    nominal must not change `stats`, X or U — in particular not the status, `acc` or `accp` of a trajectory that leaves early.
    (The large-batch paths are forced at B = 70 / 40 through their knobs.)  And the common result is the oracle's."""
    _identity(what, name, common, knob, values, hip, oracle, monkeypatch)


def _identity(what, name, common, knob, values, hip, oracle, monkeypatch):
    case = F.CASES[name]
    out = []
    for v in values:
        def run():
            with monkeypatch.context() as mp:
                for k in EXTRA_KNOBS:
                    mp.delenv(k, raising=False)
                for k, val in {**common, knob: v}.items():
                    mp.setenv(k, val)
                return solve_all(case, hip)
        out.append(with_env(monkeypatch, {}, run))
    (s0, X0, U0, i0), (s1, X1, U1, i1) = out
    idx = {"TRAJOPT_COMPACT": 2, "TRAJOPT_FWD2": 4, "TRAJOPT_ACCEPT_ROLL_MIN": 6, "TRAJOPT_LS_REPACK": 7, "TRAJOPT_REPACK": 7}[knob]
    assert i0[idx] != i1[idx], f"{what}: the knob changed nothing in to_solver_path ({i0} / {i1})"
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(X0, X1)
    np.testing.assert_array_equal(U0, U1)
    assert_case_solve(name, s0, X0, U0, oracle)


# --------------------------------------------------------------------------------------------------------------- 5. one NaN pivot
@pytest.mark.parametrize("path", ["lane", "scan", "coop", "mfma"])
def test_one_nan_pivot(path, hip, oracle, monkeypatch):
    """One NaN in one state of one knot of one trajectory (T.initial_states after the rollout), then expand and backwardpass: that
    trajectory's pivots are NaN at every regularisation level, so its pass must end the way the oracle's does — rho past bp_reg_max,
    a failed pass — after the bounded number of restarts of this file's docstring, and every other trajectory's gains must equal
    those of the clean batch bit for bit.

    Of the two -fno-honor-nans translation units this covers ONE: the "scan" row runs k_expand_backward_scan of ops_small_scan.hip, whose
    positive-definiteness test works on bit patterns (common.h not_positive).  The "lane" row does NOT cover the other: it runs
    k_expand_lane of ops_small_lane.hip, which tests no pivot, and k_backward_lane, which is compiled with the normal flags.  The
    not_positive of ops_small_lane.hip sits in lane_riccati_knot inside k_expand_backward_lane; that kernel runs inside solves only,
    whose rollouts turn a NaN into STATE_LIMIT / MAXIMUM_COST before any backward pass, so no NaN can be handed to it through the
    API: NOT COVERED, ops_small_lane.hip's not_positive still has no NaN test."""
    case = F.CASES["cartpole_levels"]
    env, want = PHASE_PATHS[path]
    bad, knot = 37, 23

    def run(lib, poison):
        p = case.build(lib)
        if lib is hip:
            assert_path(p, want, f"NaN on {path}")
        T.rollout(p)
        if poison:
            X = T.states(p)
            X[bad, knot, 1] = np.nan
            T.initial_states(p, X)
        I.expand(p); I.backwardpass(p)
        g = I.gains(p)
        ls, J = I.forwardpass(p)
        return g, ls, p.case_options.bp_reg_max
    clean, _, _ = with_env(monkeypatch, env, lambda: run(hip, False))
    g, ls, rmax = with_env(monkeypatch, env, lambda: run(hip, True))
    go, lso, _ = run(oracle, True)
    assert go["rho"][bad] > rmax and lso[bad] == -1            # the oracle: a failed pass
    np.testing.assert_array_equal(g["rho"], go["rho"])
    assert ls[bad] == -1
    others = np.arange(g["rho"].size) != bad
    for k in ("K", "d", "dV", "rho"):
        np.testing.assert_array_equal(g[k][others], clean[k][others], err_msg=k)
    np.testing.assert_array_equal(ls[others], lso[others])


# ------------------------------------------------------------------------------------------------- 4 (cont.): repacked working set
@pytest.mark.parametrize("what,name,common,knob,values", WORKING_SET, ids=_ids(WORKING_SET))
def test_repacked_working_set_on_failing_batches(what, name, common, knob, values, hip, oracle, monkeypatch):
    """The dense working set of the fused lane path (k_repack_*), allowed from 8 trajectories on so that a batch of 70 moves several
    times while trajectories leave it with REGULARIZATION_MAX / NO_PROGRESS / MAXIMUM_COST: bit-identical to the solve that never
    moves anything, and the oracle's result."""
    _identity(what, name, common, knob, values, hip, oracle, monkeypatch)
