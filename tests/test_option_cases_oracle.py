"""Vets the rows of tests/option_cases.py on the CPU oracle alone, before any GPU kernel is held to them: every option of
to_solver_opts that the kernels read has a row on a small model (and, but for the three polish options, on the Quadrotor) on which it
changes the solve; penalty_max and dual_max demonstrably bind; every integer survives last-bit changes of the inputs; and the three
restatements of option_cases (step sizes, regularisation ladder, dual update) — which go through no solver code of the oracle's,
so that oracle and kernels cannot be wrong together — hold on the oracle's own phase outputs."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import failure_cases as F
import option_cases as O

NAMES = list(O.ROWS)
ILQR = O.ILQR_SMALL + O.ILQR_QUADROTOR


def test_every_option_has_its_rows(oracle):
    """Each iLQR / AL option on a small model AND on the Quadrotor, each polish option on a small model."""
    for quadrotor in (False, True):
        have = set(o for r in O.ROWS.values() if r.quadrotor == quadrotor for o in r.options)
        want = set(O.OPTIONS_ILQR + O.OPTIONS_AL + (() if quadrotor else O.OPTIONS_PN))
        assert want <= have, f"no {'Quadrotor' if quadrotor else 'small-model'} row for {sorted(want - have)}"
    default = T.SolverOptions(lib=oracle)
    for r in O.ROWS.values():
        for k, v in r.overrides.items():
            assert getattr(default, k) != v, f"{r.name}: {k} = {v} is the default"


@pytest.mark.parametrize("name", NAMES)
def test_the_option_bites_and_the_clamps_bind(name, oracle):
    row = O.ROWS[name]
    d = O.differs(row, oracle)
    st, X, U, lams, o = O.oracle_solve(row, oracle)
    p = row.build(oracle)
    assert p.B <= 70 and p.N <= 41
    print(f"\n{name}: the override changes {int(d.sum())} of {d.size} trajectories")
    assert d.sum() >= 3
    if "penalty_max" in row.overrides:
        hit = st["penalty_max"] == row.overrides["penalty_max"]
        print(f"{name}: stats['penalty_max'] == {row.overrides['penalty_max']} on {int(hit.sum())} trajectories")
        assert hit.sum() >= 3 and (st["penalty_max"] <= row.overrides["penalty_max"]).all()
    if "dual_max" in row.overrides:
        dm = row.overrides["dual_max"]
        hit = O.at_clamp(p, lams, dm)
        print(f"{name}: a dual at +-{dm} on {int(hit.sum())} trajectories")
        assert hit.sum() >= 3
        for i, lam in enumerate(lams):
            if O.clampable(p, i):
                assert (np.abs(lam) <= dm).all()
            else:
                # the cone duals are projected, not clamped: they have to exceed dual_max, or the row could not tell
                beyond = (np.abs(lam) > dm).reshape(p.B, -1).any(axis=1)
                print(f"{name}: cone duals beyond dual_max on {int(beyond.sum())} trajectories (largest {np.abs(lam).max():.3g})")
                assert beyond.sum() >= 3
    if row.base == "quadrotor_cone":
        assert any(not O.clampable(p, i) for i in range(len(lams))) and any(O.clampable(p, i) for i in range(len(lams)))


@pytest.mark.parametrize("name", NAMES)
def test_integers_survive_last_bit_changes_of_the_inputs(name, oracle):
    """The trajectories whose integers change under any shift of failure_cases.ULPS, or whose values move by more than 1e-8, leave the
    row's mask; the mask keeps at least 90 % of the batch and at least 3 of the trajectories on which the option bites."""
    row = O.ROWS[name]
    mask, unstable = O.stability(row, oracle)
    d = O.differs(row, oracle)
    print(f"\n{name}: {int(unstable.sum())} trajectories with unstable integers, the mask drops {int((~mask).sum())} of {mask.size}: {np.where(~mask)[0]}")
    assert not (mask & unstable).any()
    assert (~mask).sum() <= 0.1 * mask.size
    assert (d & mask).sum() >= 3


@pytest.mark.parametrize("name", ILQR)
def test_step_sizes(name, oracle):
    row = O.ROWS[name]
    fp = O.oracle_first_pass(row, oracle)
    o = fp["prob"].case_options
    idx = O.assert_step_sizes(fp, o.line_search_decrease_factor, name)
    print(f"\n{name}: accepted indices {dict(zip(*np.unique(idx, return_counts=True)))}")
    if "line_search_decrease_factor" in row.overrides:
        # an index >= 2, or f is indistinguishable from other values (a search of two step sizes has index 1 at the most)
        assert idx.max() >= min(2, o.iterations_linesearch - 1)
        # ... and the default factor would not pass
        with pytest.raises(AssertionError):
            O.assert_step_sizes(fp, 0.5, name)
    if name == "quadrotor_ls_0.8_deep":
        assert (idx >= 4).sum() >= 3      # past the first round of any candidate width up to 4


@pytest.mark.parametrize("name", ILQR)
def test_regularisation_ladder(name, oracle):
    row = O.ROWS[name]
    fp = O.oracle_first_pass(row, oracle)
    o = fp["prob"].case_options
    levels, nfail = O.assert_ladder(fp, o, name)
    print(f"\n{name}: levels {levels}, {nfail} failed searches")
    if "bp_reg_fp" in row.overrides:
        assert nfail >= 3
    if set(row.overrides) & {"bp_reg_increase_factor", "bp_reg_min", "bp_reg_initial"}:
        assert sum(1 for r in levels if r > 0) >= 1, "no trajectory restarts: the ladder is not exercised"
        default = T.SolverOptions(lib=oracle)
        mine, base = O.reg_ladder(o)[0], O.reg_ladder(default)[0]
        if "bp_reg_initial" not in row.overrides:
            assert set(mine) & set(base) == {0.0}
        # the levels the row shows are no members of the default ladder
        assert not (set(levels) - {0.0}) & set(base)


@pytest.mark.parametrize("name", ["levels_reg_factor", "levels_reg_min", "levels_reg_initial"])
def test_ladder_rows_against_the_float128_riccati(name, oracle):
    """The float128 restatement of the backward pass with its restart rule (failure_cases.riccati_with_restarts), run with the row's
    factor / minimum / initial value: rho exactly the oracle's for every trajectory, every level it tried a member of the ladder."""
    row = O.ROWS[name]
    p = row.build(oracle)
    o = p.case_options
    T.rollout(p)
    I.expand(p)
    A, Bm = I.dynamics_jacobians(p)
    E = I.cost_expansion(p)
    I.backwardpass(p)
    g = I.gains(p)
    tried = set()
    rho, drho = o.bp_reg_initial, 0.0
    while rho <= o.bp_reg_max:
        tried.add(rho)
        rho, drho = O.reg_increase(o, rho, drho)
    for b in range(p.B):
        r = F.riccati_with_restarts(A[b], Bm[b], {k: v[b] for k, v in E.items()}, o.bp_reg_initial, 0.0, o)
        assert r["rho"] == g["rho"][b], f"trajectory {b}: rho {r['rho']} vs {g['rho'][b]} (levels tried {r['rhos']})"
        assert set(r["rhos"]) <= tried, f"trajectory {b}: levels {r['rhos']}"


@pytest.mark.parametrize("name", O.AL)
def test_dual_updates(name, oracle):
    row = O.ROWS[name]
    du = O.oracle_duals(row, oracle, O.DUAL_CALLS)
    o = du["prob"].case_options
    mu_bound, lam_bound = O.assert_dual_updates(du, o, name)
    print(f"\n{name}: after {O.DUAL_CALLS} dual updates the penalty clamp binds on {int(mu_bound.sum())}, a dual clamp on {int(lam_bound.sum())} trajectories")
    if "penalty_max" in row.overrides:
        assert mu_bound.sum() >= 3
    if "dual_max" in row.overrides:
        assert lam_bound.sum() >= 3
    if set(row.overrides) & {"penalty_initial", "penalty_scaling"}:
        default = T.SolverOptions(lib=oracle)
        mu = du["steps"][-1][0][1]
        assert (mu != default.penalty_initial * default.penalty_scaling ** O.DUAL_CALLS).all()


def test_r_threshold_row_leaves_through_the_rate_exit(oracle):
    """The base run of the polish row holds a trajectory that leaves a projection by the convergence-rate break (the oracle's trace),
    and with the row's threshold the trace of at least 3 trajectories changes."""
    from oracle_binding import pn_trace
    row = O.ROWS["pn_r_threshold"]
    traces = []
    for override in (False, True):
        p = row.solve(oracle, override=override)[3]
        traces.append([pn_trace(p, b) for b in range(p.B)])
    base, mine = traces
    rate = [b for b, tr in enumerate(base) if any(why == "rate" for _, _, why in tr)]
    print(f"\npn_r_threshold: rate exits of the base run on trajectories {rate}; traces change on {[b for b in range(len(base)) if base[b] != mine[b]]}")
    assert rate
    assert sum(base[b] != mine[b] for b in range(len(base))) >= 3
    assert any(base[b] != mine[b] for b in rate)
