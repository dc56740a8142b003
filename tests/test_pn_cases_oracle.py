"""Vets the polish cases of tests/pn_cases.py on the CPU oracle alone, before the kernel source (tests/test_pn_host.py) or a GPU
(tests/test_gpu_pn_blocks.py) is held to them: every rung of the ladder really has the stride and the active blocks it is named for,
every exit of the polish occurs, every integer and every exit class survives starts moved by one ulp either way and the oracle's
second factorisation order (ORACLE_PN_DENSE), and the spread of the oracle's own results over those runs gives the tolerance of the
trajectories that Newton does not contract (the ones that end PROJECTION_FAIL).  All selection happens here and in pn_cases.py (a
trajectory that is not stable is replaced there by another seed): the GPU tests exclude nothing."""
import os

import numpy as np
import pytest

import trajopt_amd as T
import pn_cases as P

NAMES = list(P.CASES)
RUNS = (("+1 ulp", 1, False), ("-1 ulp", -1, False), ("dense", 0, True))


def _polish(case, oracle, ulp=0, dense=False):
    old = os.environ.pop("ORACLE_PN_DENSE", None)
    if dense:
        os.environ["ORACLE_PN_DENSE"] = "1"
    try:
        out = case.polish(oracle, ulp=ulp)
    finally:
        os.environ.pop("ORACLE_PN_DENSE", None)
        if old is not None:
            os.environ["ORACLE_PN_DENSE"] = old
    out["labels"] = P.classify(case, out, out["prob"])
    return out


@pytest.fixture(scope="module")
def vetted(oracle):
    res = {}
    for name in NAMES:
        case = P.CASES[name]
        res[name] = (_polish(case, oracle), [(tag, _polish(case, oracle, ulp, dense)) for tag, ulp, dense in RUNS])
    return res


def spread_of(base, others, sel):
    """largest difference of X, U and c_max of the trajectories `sel` between the base run and the others (NaN equals NaN)"""
    worst = 0.0
    for _, o in others:
        for k in ("X", "U", "c_max"):
            a, b = base[k][sel], o[k][sel]
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
            d = np.abs(a - b)
            worst = max(worst, float(np.nanmax(d)) if d.size and not np.all(np.isnan(d)) else 0.0)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_case_on_the_oracle(name, oracle, vetted):
    case = P.CASES[name]
    base, others = vetted[name]
    NB, nb, stride = P.strides(case, case.build(oracle))
    failing = base["status"] != T.capi.SOLVE_SUCCEEDED
    s_fail, s_conv = spread_of(base, others, failing), spread_of(base, others, ~failing)
    classes = sorted(set().union(*base["labels"]))
    print(f"\n{name}: NB = {NB}, largest nb = {int(nb.max())} (nb per knot {[int(v) for v in nb]}), exits {classes}, projections "
          f"{base['iterations_pn'].tolist()}, status {base['status'].tolist()}; oracle spread over {[t for t, _ in others]}: "
          f"{s_fail:.3e} on the {int(failing.sum())} PROJECTION_FAIL trajectories (tolerance 16 x = {max(16 * s_fail, 1e-12):.3e}, recorded "
          f"{case.tol}), {s_conv:.3e} on the converged ones")
    # the rung is really hit
    assert NB == case.NB and int(nb.max()) == case.nb
    if case.terminal_nb is not None:
        assert int(nb[-1]) == case.terminal_nb
    assert len(set(int(v) for v in nb)) >= 3 and len(set(int(v) for v in stride)) >= 3   # consecutive records differ in nb and in stride
    # the exits it is meant to show
    for c in case.expect:
        assert c in classes, f"no trajectory of {name} leaves the polish by '{c}'"
    if name in P.LADDER:
        assert not failing.any() and base["c_max"].max() <= 1e-6 and np.all(base["iterations_pn"] >= 1)
    else:
        assert (~failing).any(), "an exit case holds healthy trajectories too"
    # integers and exit classes survive last-bit changes of the start and the other factorisation order
    for tag, o in others:
        np.testing.assert_array_equal(o["status"], base["status"], err_msg=f"status, {tag}")
        np.testing.assert_array_equal(o["iterations_pn"], base["iterations_pn"], err_msg=f"iterations_pn, {tag}")
        assert o["labels"] == base["labels"], f"exit classes, {tag}: {o['labels']} vs {base['labels']}"
    # converged trajectories are held to 1e-8 on every side: the oracle's own spread has to be far inside that
    assert 16 * s_conv <= 1e-8
    if failing.any():
        assert case.tol is not None and max(16 * s_fail, 1e-12) <= case.tol, f"{name}: record tol >= {max(16 * s_fail, 1e-12):.2e} in pn_cases.TOL"
        assert case.tol <= 1e-6, "a tolerance this wide compares nothing: replace the case"


def test_every_exit_of_the_polish_occurs(vetted):
    seen = set()
    for name in P.EXITS:
        seen |= set().union(*vetted[name][0]["labels"])
    assert {"converged", "budget", "factor", "nan", "linesearch", "rate"} <= seen, seen
    # ... with n_steps of 0 and of 1, and the refinement limit (PN_REFINEMENTS steps on one linearisation) among the traces
    from oracle_binding import pn_trace
    for name, n_steps in (("budget_n_steps0", 0), ("budget_n_steps1", 1)):
        b = vetted[name][0]
        assert any("budget" in L for L in b["labels"]) and b["iterations_pn"].max() == n_steps + 1
    why = {w for name in P.EXITS for b in range(P.CASES[name].B) for _, _, w in pn_trace(vetted[name][0]["prob"], b)}
    assert "refinements" in why


def test_the_ladder_covers_every_path(oracle):
    """strides on both sides of every limit that chooses a code path of csrc/k_pn.h, computed from the limits the source exports"""
    L = P.limits()
    NBs = sorted(P.CASES[n].NB for n in P.LADDER if n.startswith("quadrotor"))
    q = P.rungs(12, 16)
    for want in (q["last_reg"], q["first_generic"], q["last_staged_factor"], q["first_unstaged_factor"], L["nb_limit"] - 1, L["nb_limit"]):
        assert want in NBs, (want, NBs)
    assert q["last_reg"] ** 2 <= 64 * L["pf"] < q["first_generic"] ** 2 and q["last_reg"] <= L["nbr"]
    assert (q["last_staged_factor"] - 12) * 16 <= 64 * L["pf"] < (q["first_unstaged_factor"] - 12) * 16
    kib = [NB for NB in NBs if P.lds_bytes(12, 4, NB) <= 65536]
    assert max(kib) + 1 in NBs and P.lds_bytes(12, 4, max(kib) + 1) > 65536      # 42 | 43
    assert (P.lds_bytes(12, 4, 42), P.lds_bytes(12, 4, 43), P.lds_bytes(12, 4, 44)) == (63312, 65872, 68480)
    # the fullest knot at knot 1 and at knot N-1, a knot without candidate rows next to it; nb = 28 on an interior knot, >= 24 at the end
    cases = [P.CASES[n] for n in P.LADDER]
    fullest = {}
    for c in cases:
        stride = P.strides(c, c.build(oracle))[2]
        fullest.setdefault(int(np.argmax(stride)) if int(np.argmax(stride)) < c.N - 1 else -1, []).append(stride)
    assert 1 in fullest and -1 in fullest and any(1 < k for k in fullest)
    assert any(st[0] == st[2] == st.min() for st in fullest[1])                  # no candidate row on either side of the fullest knot
    assert any(c.nb >= 28 for c in cases) and any((c.terminal_nb or 0) >= 24 for c in cases)
    small = [P.CASES[n] for n in P.LADDER if not n.startswith("quadrotor")]
    assert any(c.NB == L["nb_limit"] and c.model.dims() == (4, 1) for c in small)
    assert any(c.NB >= 30 and c.model.dims() == (6, 3) for c in small)
    assert any(c.N > 64 and c.NB > q["last_reg"] for c in small)


@pytest.mark.parametrize("name", list(P.FLEET))
def test_fleet_variants_on_the_oracle(name, oracle):
    """the cases that also run with one plant per trajectory: integers stable, the spread of the values inside the tolerances"""
    case = P.CASES[name]
    models = P.fleet_models(case)
    base = P.polish_fleet(case, oracle, models)
    failing = base["status"] != T.capi.SOLVE_SUCCEEDED
    others = []
    for tag, ulp, dense in RUNS:
        if dense:
            os.environ["ORACLE_PN_DENSE"] = "1"
        try:
            others.append((tag, P.polish_fleet(case, oracle, models, ulp=ulp)))
        finally:
            os.environ.pop("ORACLE_PN_DENSE", None)
    for tag, o in others:
        np.testing.assert_array_equal(o["status"], base["status"], err_msg=tag)
        np.testing.assert_array_equal(o["iterations_pn"], base["iterations_pn"], err_msg=tag)
    s_fail, s_conv = spread_of(base, others, failing), spread_of(base, others, ~failing)
    print(f"\n{name} with one plant per trajectory: projections {base['iterations_pn'].tolist()}, status {base['status'].tolist()}, spread "
          f"{s_fail:.3e} (PROJECTION_FAIL) / {s_conv:.3e} (converged)")
    assert (~failing).any() and np.all(base["iterations_pn"][~failing] >= 1) and 16 * s_conv <= 1e-8
    if failing.any():
        assert max(16 * s_fail, 1e-12) <= case.tol
    if name == "nan_state":
        assert np.isnan(base["c_max"]).sum() == 1


@pytest.mark.parametrize("name", list(P.ALTRO))
def test_altro_variants_on_the_oracle(name, oracle):
    """the exit cases that also go through to_altro_solve: the polish runs, the integers are stable, a NaN control keeps its trajectory out"""
    case = P.CASES[name]
    base = P.altro(case, oracle, nan_control=P.ALTRO[name])
    print(f"\n{name} through ALTRO: iterations {base['iterations'].tolist()}, projections {base['iterations_pn'].tolist()}, status {base['status'].tolist()}, "
          f"c_max {base['c_max'].tolist()}")
    assert base["iterations_pn"].max() >= 1
    for ulp in (1, -1):
        o = P.altro(case, oracle, ulp=ulp, nan_control=P.ALTRO[name])
        for k in ("status", "iterations", "iterations_outer", "iterations_pn"):
            np.testing.assert_array_equal(o[k], base[k], err_msg=f"{k}, {ulp:+d} ulp")
    if P.ALTRO[name] is not None:
        b = P.ALTRO[name][0]
        assert np.isnan(base["c_max"][b]) and base["iterations_pn"][b] == 0 and np.isnan(base["c_max"]).sum() == 1
    else:
        assert np.any(base["status"] == T.capi.PROJECTION_FAIL)
