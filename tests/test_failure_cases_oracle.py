"""Vets the failing batches of tests/failure_cases.py on the CPU oracle alone, before any GPU kernel is held to them: every class a
case is meant to exercise is populated (in both tiles, three classes in one tile), every decision of the backward pass has a margin
a second implementation cannot legitimately fall on the other side of, every integer survives last-bit changes of the inputs, and
the trajectories whose values do not (value_mask) are few."""
import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
import failure_cases as F

NAMES = list(F.CASES)


@pytest.fixture(scope="module")
def classified(oracle):
    return {name: F.classify(F.CASES[name], oracle) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_class_mix(name, classified):
    case = F.CASES[name]
    labels, info = classified[name]
    hist = F.histogram(labels)
    B = len(labels)
    tiles = [labels[t0:t0 + 64] for t0 in range(0, B, 64)]
    print(f"\n{name} (B = {B}): {hist}; per tile: {[F.histogram(t) for t in tiles]}")
    for c in case.expect:
        assert hist.get(c, 0) >= 3, f"class {c} holds {hist.get(c, 0)} trajectories"
        for i, t in enumerate(tiles):
            assert any(c in L for L in t), f"class {c} does not occur in tile {i}"
    assert max(sum(any(c in L for L in t) for c in case.expect) for t in tiles) >= min(3, len(case.expect))
    present = set(int(s) for s in info["stats"]["status"])
    assert set(case.statuses) <= present, f"statuses {case.statuses} expected, {present} present"
    assert B > 64 or not case.small           # the small models cover a full tile and a ragged one


@pytest.mark.parametrize("name", [n for n in NAMES if F.CASES[n].small])
def test_decision_margins(name, oracle):
    """The float128 restatement of the backward pass agrees with the oracle (rho exactly, K / d / dV at 1e-10), and every pivot it
    accepted or rejected is at least 1e-6 of the largest term of that Quu + rho I away from zero: arithmetic that differs in the
    last bits cannot decide differently.  A condition on the INPUTS of the cases, not a tolerance."""
    case = F.CASES[name]
    p = case.build(oracle)
    T.rollout(p)
    I.expand(p)
    A, Bm = I.dynamics_jacobians(p)
    E = I.cost_expansion(p)
    o = p.case_options
    I.backwardpass(p)
    g = I.gains(p)
    worst = np.inf
    for b in range(p.B):
        r = F.riccati_with_restarts(A[b], Bm[b], {k: v[b] for k, v in E.items()}, o.bp_reg_initial, 0.0, o)
        assert r["rho"] == g["rho"][b], f"trajectory {b}: rho {r['rho']} vs {g['rho'][b]} (levels tried {r['rhos']})"
        assert r["failed"] == bool(g["rho"][b] > o.bp_reg_max)
        for v, scale, ok in r["pivots"]:
            worst = min(worst, abs(v) / scale)
            assert abs(v) >= 1e-6 * scale, f"trajectory {b}: pivot {v} (scale {scale}, accepted {ok}) is too close to zero"
        if not r["failed"]:
            np.testing.assert_allclose(g["K"][b], r["K"], rtol=1e-10, atol=1e-10 * np.abs(r["K"]).max())
            np.testing.assert_allclose(g["d"][b], r["d"], rtol=1e-10, atol=1e-10 * max(np.abs(r["d"]).max(), 1e-300))
            np.testing.assert_allclose(g["dV"][b], r["dV"], rtol=1e-10)
    print(f"\n{name}: smallest |pivot| / scale = {worst:.3e}")


@pytest.mark.parametrize("name", NAMES)
def test_integers_survive_last_bit_changes_of_the_inputs(name, oracle, classified):
    case = F.CASES[name]
    _, info = classified[name]
    fp, st = info["first"], info["stats"]
    for ulp in F.ULPS:
        fp2 = case.first_pass(oracle, ulp=ulp)
        np.testing.assert_array_equal(fp2["rho"], fp["rho"], err_msg=f"rho after the first pass, {ulp:+d} ulp")
        np.testing.assert_array_equal(fp2["ls"], fp["ls"], err_msg=f"first line-search index, {ulp:+d} ulp")
        st2 = case.solve(oracle, ulp=ulp)[0]
        for k in ("status", "iterations", "iterations_outer", "iterations_pn"):
            np.testing.assert_array_equal(st2[k], st[k], err_msg=f"{k}, {ulp:+d} ulp")


@pytest.mark.parametrize("name", NAMES)
def test_value_mask(name, oracle, classified):
    case = F.CASES[name]
    labels, _ = classified[name]
    mask = F.value_mask(case, oracle)
    print(f"\n{name}: value mask drops {int((~mask).sum())} of {mask.size}: {np.where(~mask)[0]}")
    assert (~mask).sum() <= 0.1 * mask.size
    for c in case.expect:
        assert any(c in L for L, keep in zip(labels, mask) if keep), f"the mask empties class {c}"


def test_both_sources_of_regularization_max(oracle, classified):
    """forward_finish ends a trajectory REGULARIZATION_MAX from two places: a backward pass that ran into bp_reg_max (bpfail), and a
    failed line search whose regularisation increase carries rho past bp_reg_max.  cartpole_regmax, replayed phase by phase on the
    oracle, holds at least 3 trajectories of each, and together they are exactly the status-10 trajectories of its solve."""
    case = F.CASES["cartpole_regmax"]
    p = case.build(oracle)
    rmax = p.case_options.bp_reg_max
    T.rollout(p)
    left = np.zeros(p.B, int)          # 0: still iterating, 1: left after a failed backward pass, 2: after a failed line search
    when = np.full(p.B, -1)
    for it in range(p.case_options.iterations):
        I.expand(p); I.backwardpass(p)
        bp = (I.gains(p)["rho"] > rmax) & (left == 0)
        left[bp], when[bp] = 1, it
        ls, _ = I.forwardpass(p)
        fs = (ls < 0) & (I.gains(p)["rho"] > rmax) & (left == 0)
        left[fs], when[fs] = 2, it
    print(f"\ncartpole_regmax: {int((left == 1).sum())} leave after a failed backward pass, {int((left == 2).sum())} after a failed line search "
          f"(trajectories {np.where(left == 2)[0]}, iterations {when[left == 2]})")
    np.testing.assert_array_equal(left > 0, classified["cartpole_regmax"][1]["stats"]["status"] == T.capi.REGULARIZATION_MAX)
    assert (left == 1).sum() >= 3 and (left == 2).sum() >= 3
