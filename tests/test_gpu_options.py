"""The rows of tests/option_cases.py — every solver option the kernels read, off its default — on every kernel path, against the
CPU oracle and against the three restatements of option_cases that go through no solver code.  tests/test_option_cases_oracle.py vets
the rows on the oracle alone (the option bites, penalty_max and dual_max bind, integers stable under last-bit changes of the inputs,
value mask); this file holds the kernels to them: single phases, the dual-update phases, short solves, the bit identities between
kernel paths, and options handed to a handle after it was created.

Trip count of the restart loops: the argument in the docstring of tests/test_gpu_failure_paths.py holds for any factor f > 1 (every
restart follows a reg_increase, which multiplies rho by at least f from the second failure on, and only happens while rho <=
bp_reg_max).  The rows here use f = 1.6 and f = 2.5 (>= 1.3) and bp_reg_max / bp_reg_min <= 1e16, so a pass restarts at most
1 + log(1e16) / log(1.6) = 80 times (42 with f = 2.5), each restart of at most N - 1 = 40 knots.  No input of this file can make a kernel
spin; every row is a validated option set."""
import numpy as np
import pytest

import trajopt_amd as T
import failure_cases as F
import option_cases as O
from test_gpu_failure_paths import PHASE_PATHS, SOLVE_PATHS, EXTRA_KNOBS, with_env, assert_path, solver_path

pytestmark = pytest.mark.gpu
ROWS = O.ROWS


def _has(row, path):
    """The paths the row's model has: the Quadrotor keeps its default backward kernel (forward kernels only), the scan kernel takes
    unconstrained problems only, the 2-D double integrator has no MFMA backward pass compiled, the polish is one kernel."""
    if row.pn:
        return path == "default"
    if row.quadrotor:
        return path in ("default", "fwd1", "fwd2")
    if path == "scan" and row.solver != "ilqr":
        return False
    return path != "mfma" or not row.base.startswith("di2")


# ------------------------------------------------------------------------------------------------------------- 1. single phases
PHASE_ROWS = [(n, p) for n in O.ILQR_SMALL for p in ("coop", "lane", "mfma", "scan")] + [(n, "default") for n in O.ILQR_QUADROTOR]


@pytest.mark.parametrize("name,path", PHASE_ROWS)
def test_one_iteration_phase_by_phase(name, path, hip, oracle, monkeypatch):
    """rollout / expand / backwardpass / gains / forwardpass with the row's options on the backward kernel the knobs select (asserted
    with to_solver_path), against the oracle at the tolerances of test_gpu_failure_paths.test_one_iteration_phase_by_phase: rho bit
    for bit after the backward pass and again after the forward pass, K / d at rtol 1e-7 / atol 1e-9, dV at 1e-8, line-search index
    equal, J at 1e-8 — and the step-size and ladder restatements on the GPU's own outputs."""
    row = ROWS[name]
    env, want = PHASE_PATHS.get(path, ({}, (1, 0, 0)))     # the Quadrotor's default is the MFMA kernel

    def run():
        fp = row.first_pass(hip)
        assert_path(fp["prob"], want, f"{name} on {path}")
        return fp
    fp = with_env(monkeypatch, env, run)
    o = O.oracle_first_pass(row, oracle)
    g, go = fp["gains"], o["gains"]
    np.testing.assert_array_equal(g["rho"], go["rho"])
    ok = ~o["bpfail"]
    np.testing.assert_allclose(g["K"][ok], go["K"][ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["d"][ok], go["d"][ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(g["dV"][ok], go["dV"][ok], rtol=1e-8)
    np.testing.assert_array_equal(fp["ls"], o["ls"])
    np.testing.assert_allclose(fp["J"], o["J"], rtol=1e-8)
    np.testing.assert_array_equal(fp["rho_after"], o["rho_after"])
    np.testing.assert_allclose(fp["X"], o["X"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(fp["U"], o["U"], rtol=1e-7, atol=1e-9)
    # no step where the search failed
    lsf = fp["ls"] < 0
    np.testing.assert_array_equal(fp["X"][lsf], fp["X0"][lsf]); np.testing.assert_array_equal(fp["U"][lsf], fp["U0"][lsf])
    opts = fp["prob"].case_options
    idx = O.assert_step_sizes(fp, opts.line_search_decrease_factor, f"{name} on {path}")
    levels, nfail = O.assert_ladder(fp, opts, f"{name} on {path}")
    print(f"\n{name} on {path}: accepted indices {dict(zip(*np.unique(idx, return_counts=True)))}, levels {levels}, {nfail} failed searches")


# ----------------------------------------------------------------------------------------------------------- 2. dual-update phases
@pytest.mark.parametrize("name", O.AL)
def test_dual_update_phases(name, hip, oracle):
    """k x I.dual_update (k_dual_update) from zero duals on the rollout of the initial controls: the penalties bit-equal to the
    oracle's, the duals at rtol 1e-11 / atol 1e-13 with the entries at a clamp bit-equal, and the numpy restatement on the GPU's outputs."""
    row = ROWS[name]
    du, duo = row.duals_after(hip, O.DUAL_CALLS), O.oracle_duals(row, oracle, O.DUAL_CALLS)
    o = du["prob"].case_options
    for j, (step, stepo) in enumerate(zip(du["steps"], duo["steps"])):
        for i, ((lam, mu), (lamo, muo)) in enumerate(zip(step, stepo)):
            np.testing.assert_array_equal(mu, muo, err_msg=f"{name}: penalty of constraint {i} after {j} calls")
            np.testing.assert_allclose(lam, lamo, rtol=1e-11, atol=1e-13, err_msg=f"{name}: duals of constraint {i} after {j} calls")
            if O.clampable(du["prob"], i):
                hit = np.abs(lamo) == o.dual_max
                np.testing.assert_array_equal(lam[hit], lamo[hit], err_msg=f"{name}: duals of constraint {i} at the clamp after {j} calls")
    mu_bound, lam_bound = O.assert_dual_updates(du, o, name)
    if "penalty_max" in row.overrides:
        assert mu_bound.sum() >= 3
    if "dual_max" in row.overrides:
        assert lam_bound.sum() >= 3


# -------------------------------------------------------------------------------------------------------------- 3. short solves
SOLVE_ROWS = [(n, p) for n, r in ROWS.items() for p in SOLVE_PATHS if _has(r, p)]


def assert_row_solve(row, st, X, U, lams, oracle):
    """Integers equal to the oracle's for every trajectory; stats["penalty_max"] bit-equal; X, U, cost at 1e-6 on the trajectories of
    the row's mask; the final duals that sit at the clamp bit-equal there."""
    sto, Xo, Uo, lamo, o = O.oracle_solve(row, oracle)
    for k in O.INTS:
        np.testing.assert_array_equal(st[k], sto[k], err_msg=k)
    assert st["total_iterations"] == sto["total_iterations"]
    np.testing.assert_array_equal(st["penalty_max"], sto["penalty_max"])
    m = O.stability(row, oracle)[0]
    ex, eu = F.trajectory_error(X, Xo), F.trajectory_error(U, Uo)
    print(f"\n{row.name}: largest error on the {int(m.sum())} masked trajectories X {ex[m].max():.2e} U {eu[m].max():.2e}, "
          f"on the {int((~m).sum())} others X {ex[~m].max(initial=0):.2e} U {eu[~m].max(initial=0):.2e}")
    assert F.trajectories_close(X, Xo, 1e-6)[m].all(), f"X: trajectories {np.where(~F.trajectories_close(X, Xo, 1e-6) & m)[0]}"
    assert F.trajectories_close(U, Uo, 1e-6)[m].all(), f"U: trajectories {np.where(~F.trajectories_close(U, Uo, 1e-6) & m)[0]}"
    np.testing.assert_allclose(st["cost"][m], sto["cost"][m], rtol=1e-6)
    if row.solver in ("altro", "pn"):
        np.testing.assert_allclose(st["c_max"][m], sto["c_max"][m], rtol=1e-3, atol=1e-9)
    if "dual_max" in row.overrides:
        nhit = 0
        for i, (lam, lo) in enumerate(zip(lams, lamo)):
            hit = (np.abs(lo) == o.dual_max) & m.reshape((-1,) + (1,) * (lo.ndim - 1))
            np.testing.assert_array_equal(lam[hit], lo[hit], err_msg=f"final duals of constraint {i} at the clamp")
            nhit += int(hit.sum())
        assert nhit >= 3


@pytest.mark.parametrize("name,path", SOLVE_ROWS)
def test_short_solves(name, path, hip, oracle, monkeypatch):
    """The rows as iLQR / AL / ALTRO / polish solves on every solve-loop path their model has: k_outer_decide / k_outer_update with
    penalty_max and dual_max binding, forward_finish of both forward kernels with bp_reg_fp and gradient_tolerance, every backward
    kernel's restart loop with a non-default factor and minimum."""
    env, want = SOLVE_PATHS[path]
    row = ROWS[name]

    def run():
        st, X, U, p = row.solve(hip)
        # (the Quadrotor keeps its default backward kernel: only the forward kernel of its rows is asserted)
        assert_path(p, want if not row.quadrotor or path in ("fwd1", "fwd2") else None, f"{name} on {path}")
        return st, X, U, O.final_duals(p)
    st, X, U, lams = with_env(monkeypatch, env, run)
    assert_row_solve(row, st, X, U, lams, oracle)


# ------------------------------------------------------------------------------------------------ 4. bit identities between paths
_REPACK = {"TRAJOPT_LS_DEEP": "0", "TRAJOPT_LS_CANDIDATES": "2", "TRAJOPT_FWD2": "1"}
_QUADROTOR_KNOBS = [({}, "TRAJOPT_COMPACT", ("1", "0")), ({}, "TRAJOPT_FWD2", ("0", "1")), (_REPACK, "TRAJOPT_LS_REPACK", ("0", "1")),
                    ({"TRAJOPT_FWD2": "0"}, "TRAJOPT_ACCEPT_ROLL_MIN", ("0", "1"))]
# (the Cartpole writes accepted steps through and never repacks its last line-search round: no TRAJOPT_LS_REPACK rows)
_SMALL_KNOBS = [({"TRAJOPT_BACKWARD": "lane"}, "TRAJOPT_COMPACT", ("1", "0")), ({}, "TRAJOPT_FWD2", ("0", "1")),
                ({"TRAJOPT_FWD2": "0"}, "TRAJOPT_ACCEPT_ROLL_MIN", ("0", "1"))]
IDENTITIES = ([(n, c, k, v) for n in ("quadrotor_ls_0.8_deep", "quadrotor_reg_fp", "cone_clamps") for c, k, v in _QUADROTOR_KNOBS]
              + [(n, c, k, v) for n in ("no_progress_reg_fp_0.5", "al_clamps") for c, k, v in _SMALL_KNOBS])


@pytest.mark.parametrize("name,common,knob,values", IDENTITIES, ids=[f"{n}-{k}" for n, _, k, _ in IDENTITIES])
def test_kernel_choices_are_invisible_with_non_default_options(name, common, knob, values, hip, oracle, monkeypatch):
    """Which forward kernel runs, how the line search is laid out, who owns a trajectory and how an accepted step reaches the nominal
    must not change stats, X or U with a non-default step factor, bp_reg_fp or binding clamps either: bit-identical, the knob changed
    to_solver_path, and the common result is the oracle's."""
    row = ROWS[name]
    out = []
    for v in values:
        def run():
            with monkeypatch.context() as mp:
                for k in EXTRA_KNOBS:
                    mp.delenv(k, raising=False)
                for k, val in {**common, knob: v}.items():
                    mp.setenv(k, val)
                st, X, U, p = row.solve(hip)
                return st, X, U, solver_path(p), O.final_duals(p)
        out.append(with_env(monkeypatch, {}, run))
    (s0, X0, U0, i0, l0), (s1, X1, U1, i1, l1) = out
    idx = {"TRAJOPT_COMPACT": 2, "TRAJOPT_FWD2": 4, "TRAJOPT_ACCEPT_ROLL_MIN": 6, "TRAJOPT_LS_REPACK": 7}[knob]
    assert i0[idx] != i1[idx], f"{name}: {knob} changed nothing in to_solver_path ({i0} / {i1})"
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=f"{name}, {knob}: {k}")
    np.testing.assert_array_equal(X0, X1)
    np.testing.assert_array_equal(U0, U1)
    for a, b in zip(l0, l1):
        np.testing.assert_array_equal(a, b)
    assert_row_solve(row, s0, X0, U0, l0, oracle)


# ----------------------------------------------------------------------------------------------------------- 5. options set late
def _assert_same_solve(a, b, what):
    (s0, X0, U0, _), (s1, X1, U1, _) = a, b
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(X0, X1, err_msg=what)
    np.testing.assert_array_equal(U0, U1, err_msg=what)


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.late])
def test_options_set_late(name, hip, oracle):
    """A handle created WITHOUT the row's overrides, which the solver then hands over (to_set_options), solves bit-identically to a
    handle created with them: penalty_initial, bp_reg_initial and iterations_total are read by the solve's own initialisation.  (The
    phase API keeps the rho and mu that to_create wrote; nothing is asserted about it here.)"""
    row = ROWS[name]
    fresh, late = row.solve(hip), row.solve(hip, late=True)
    _assert_same_solve(fresh, late, name)
    assert_row_solve(row, late[0], late[1], late[2], O.final_duals(late[3]), oracle)
    # ... and the late options did change the solve
    base = row.solve(hip, override=False)
    assert not all(np.array_equal(base[0][k], late[0][k]) for k in O.INTS) or not np.array_equal(base[1], late[1])


@pytest.mark.parametrize("name", ["levels_ls_0.8", "quadrotor_ls_0.8_deep"])
def test_line_search_slots_raised_late(name, hip, oracle):
    """The number of line-search candidate slots is fixed at to_create from iterations_linesearch; include/trajopt_hip.h promises that
    raising it later "works, with less concurrency": a handle created with 4 step sizes and raised to 20 solves bit-identically to a
    handle created with 20, on a row whose search goes past index 4."""
    row = ROWS[name]
    assert (O.oracle_first_pass(row, oracle)["ls"] > 4).sum() >= 3
    fresh = row.solve(hip)
    p = row.build(hip, iterations_linesearch=4)
    assert p.case_options.iterations_linesearch == 4
    s = O.SOLVERS[row.solver](p, iterations_linesearch=20).solve()
    st = {k: np.array(v).copy() for k, v in s.stats.items()}
    st["total_iterations"] = int(s.total_iterations)
    late = (st, T.states(p), T.controls(p), p)
    _assert_same_solve(fresh, late, name)
    assert_row_solve(row, st, late[1], late[2], [], oracle)
