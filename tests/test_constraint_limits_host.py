"""Per-trajectory constraint limits (to_set_constraint_limits_batch / to_get_... / to_clear_...), everything that needs no GPU: the host-only
lowering limits[q, B] -> row values [p, B] with every refusal (csrc/desc_lower.h, compiled as a program of its own — also under
AddressSanitizer + UndefinedBehaviorSanitizer), the row order held to the oracle's evaluate_constraints, the routing of a flagged handle
(csrc/path_plan.h), the ctypes / ABI / Julia mirrors, and the argument checks of the Python verbs."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import capi
from trajectoryoptimization_jl_amd import api

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
SHIM = ROOT / "tests" / "host_shim"
HEADER = (ROOT / "include" / "trajopt_hip.h").read_text()
NAMES = ("set_constraint_limits_batch", "get_constraint_limits_batch", "clear_constraint_limits_batch")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _harness(tmp_path, flags=()):
    exe = tmp_path / "constraint_limits_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "constraint_limits_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-3000:], r.stderr[-1500:])
    return r.stdout


def _rows(out, name):
    """-> p, [(b, r, idx, sgn, value)]"""
    lines = out.splitlines()
    i = next(k for k, l in enumerate(lines) if l.startswith(f"rows {name} "))
    p = int(lines[i].split()[3])
    rows = []
    for l in lines[i + 1:]:
        w = l.split()
        if len(w) != 5 or not w[0].isdigit():
            break
        rows.append((int(w[0]), int(w[1]), int(w[2]), float(w[3]), float(w[4])))
    return p, rows


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    return _harness(tmp_path_factory.mktemp("limits"))


def test_lowering_harness_under_asan_ubsan(tmp_path):
    _harness(tmp_path, SAN)


def test_refusals_class_and_message(harness_out):
    cases = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"^case (\w+) code (-?\d+) msg (.*)$", harness_out, flags=re.M)}
    want = {
        "nonfinite_bound": (capi.TO_ERR_ARGUMENT, "trajectory 1 is not finite"),
        "nan_bound": (capi.TO_ERR_ARGUMENT, "trajectory 1 is not finite"),
        "nonfinite_cone": (capi.TO_ERR_ARGUMENT, "trajectory 1 is not finite"),
        "inverted_bound": (capi.TO_ERR_ARGUMENT, "Upper bounds must be greater than or equal to lower bounds (trajectory 2)"),
        "inverted_mixed": (capi.TO_ERR_ARGUMENT, "Upper bounds must be greater than or equal to lower bounds (trajectory 1)"),
        "negative_cone": (capi.TO_ERR_ASSERTION, "Value must be greater than or equal to zero (trajectory 2)"),
        "quadratic_norm": (capi.TO_ERR_UNSUPPORTED, "BoundConstraint (its bounds) and NormConstraint with SecondOrderCone (its value) only"),
        "goal": (capi.TO_ERR_UNSUPPORTED, "BoundConstraint (its bounds) and NormConstraint with SecondOrderCone (its value) only"),
    }
    assert set(cases) == set(want)
    for k, (code, text) in want.items():
        assert cases[k][0] == code and text in cases[k][1], (k, cases[k])
    # the error classes the Python mirror raises for these codes
    assert capi._ERRORS[capi.TO_ERR_ARGUMENT] is T.ArgumentError and capi._ERRORS[capi.TO_ERR_UNSUPPORTED] is T.UnsupportedError
    assert capi._ERRORS[capi.TO_ERR_ASSERTION] is AssertionError
    # the messages carry the reference's wording; the lines are cited where the checks are made
    src = (CSRC / "desc_lower.h").read_text()
    assert "src/constraints.jl:712" in src and "src/constraints.jl:451" in src


def test_row_order_of_a_mixed_bound_against_the_oracle(harness_out, oracle):
    """The harness lowers limits for three trajectories of the bound  x4 <= v, u <= u_max, x1 >= -0.5, u >= u_min  (finite and infinite
    entries mixed) and prints its selector tables; row r of trajectory b restated from them, sgn * (z[idx] - value), is what the oracle's
    evaluate_constraints gives for a single problem built with trajectory b's bounds — in the same row order."""
    import constraint_limit_fleets as F
    p, rows = _rows(harness_out, "mixed")
    assert p == 6 and len(rows) == 18
    lim = np.zeros((3, 6)); idx = np.zeros(6, int); sgn = np.zeros(6)
    for b, r, i, s, v in rows:
        lim[b, r] = v; idx[r] = i; sgn[r] = s
    assert list(idx) == [3, 4, 5, 0, 4, 5] and list(sgn) == [1, 1, 1, -1, -1, -1]
    rng = np.random.default_rng(5)
    for b in range(3):
        x0 = np.r_[rng.uniform(-0.2, 0.2, 2), 0.0, 0.0]
        q = F.dint_problem(oracle, 1, x0, v=lim[b, 0], u_max=lim[b, 1:3], u_min=lim[b, 4:6], N=11, tf=1.0)
        T.initial_controls(q, rng.uniform(-2, 2, (1, 10, 2))); T.rollout(q)
        Z = np.concatenate([T.states(q)[0, :-1], T.controls(q)[0]], axis=1)           # [N-1, n+m]
        c = T.evaluate_constraints(q, 0)[0]                                           # [N-1, p]
        np.testing.assert_array_equal(c, sgn[None, :] * (Z[:, idx] - lim[b][None, :]))
    # ... and the convenience verb maps named bounds onto that order
    p_, cone = _rows(harness_out, "cone")
    assert p_ == 3 and [(r, i) for b, r, i, s, v in cone if b == 0] == [(0, 4), (1, 5), (2, -1)]
    assert [v for b, r, i, s, v in cone if r == 2] == [4.5, 7.5, 0.0] and all(v == 0.0 for b, r, i, s, v in cone if r < 2)


def test_routing_of_a_flagged_handle(tmp_path):
    exe = tmp_path / "constraint_limits_plan_harness"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", str(CSRC), str(SHIM / "constraint_limits_plan_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    words = r.stdout.split()
    count = lambda k: int(words[words.index(k) + 1])
    assert count("fails") == 0 and count("checks") > 10 ** 6
    # both sides were reached: unflagged handles that take the fused cooperative kernel, flagged ones on the fused lane path, in two-wave
    # workgroups and with a repacked working set in the report
    for k in ("flagged", "plain", "cleared", "fused_plain", "lane_flagged", "two_wave_flagged", "repack_flagged"):
        assert count(k) > 1000, (k, r.stdout)


def test_ctypes_signatures_and_abi_symbols():
    C = capi.C
    assert capi.HIP_ONLY["set_constraint_limits_batch"] == [capi._H, C.c_int32, capi._PD]
    assert capi.HIP_ONLY["get_constraint_limits_batch"] == [capi._H, C.c_int32, capi._PD]
    assert capi.HIP_ONLY["clear_constraint_limits_batch"] == [capi._H]
    for n in NAMES:
        assert n in capi.OPTIONAL_HIP and n not in capi.SIGNATURES      # found by symbol lookup; the oracle does not have them
        assert re.search(r"^int to_" + n + r"\(to_handle\* h", HEADER, flags=re.M), n
    assert "#define TO_ABI_VERSION 7\n" in HEADER and "#define TO_ABI_MINOR 1\n" in HEADER and capi.TO_ABI_VERSION == 7
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    assert "to_set_constraint_limits_batch" in history and "symbol lookup" in history
    for n in ("set_constraint_limits_batch", "get_constraint_limits_batch", "clear_constraint_limits_batch", "set_bounds_batch"):
        assert n in api.__all__ and callable(getattr(T, n))
    lib = CSRC / "libtrajopt_hip.so"
    if lib.exists():  # a built tree exports them (the build itself binds every name the library has)
        syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(r"\bT to_" + n + r"$", syms, flags=re.M), n


def test_julia_shim_binds_the_verbs():
    shim = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
    for verb, sym, types in (("set_constraint_limits_batch!", "to_set_constraint_limits_batch", "(Ptr{Cvoid}, Int32, Ptr{Float64})"),
                             ("get_constraint_limits_batch", "to_get_constraint_limits_batch", "(Ptr{Cvoid}, Int32, Ptr{Float64})"),
                             ("clear_constraint_limits_batch!", "to_clear_constraint_limits_batch", "(Ptr{Cvoid},)")):
        assert f"function {verb}(" in shim and f"ccall((:{sym}, lib), Cint, {types}" in shim, verb
        assert re.search(r"^export .*\b" + re.escape(verb), shim, flags=re.M), verb
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_set_constraint_limits_batch; throw_error = false)" in shim
    assert "Int32(con_id - 1)" in shim[shim.index("function set_constraint_limits_batch!"):shim.index("function clear_constraint_limits_batch!")]


def test_the_oracle_refuses_per_trajectory_limits(oracle):
    import constraint_limit_fleets as F
    p = F.cartpole_problem(oracle, 3, N=11, tf=0.5)
    for call in (lambda: T.set_constraint_limits_batch(p, 0, np.tile([3.0, -3.0], (3, 1))), lambda: T.get_constraint_limits_batch(p, 0),
                 lambda: T.clear_constraint_limits_batch(p), lambda: T.set_bounds_batch(p, 0, u_max=np.full((3, 1), 2.0))):
        with pytest.raises(T.UnsupportedError, match="to_set_constraint_limits_batch"):
            call()


class _Recorder:
    """Stands in for the library behind a problem: records what the verbs hand to it."""

    def __init__(self, prob):
        self.calls = []
        self._fn = dict.fromkeys(NAMES)
        self.prob = prob

    def call(self, name, *args):
        self.calls.append((name, args))
        return 0


def _recorded(prob):
    rec = _Recorder(prob)
    prob._lib = rec
    got = []
    prob._call = lambda name, *args: got.append((name, args[0] if args else None, np.ctypeslib.as_array(args[1], shape=(prob.B * _q(prob, args[0]),)).copy() if len(args) > 1 else None))
    return got


def _q(prob, i):
    con = prob.constraints.constraints[i]
    return con.p if con.kind == capi.CON_BOUND else 1


def test_set_bounds_batch_maps_named_bounds_onto_the_row_order(oracle):
    import constraint_limit_fleets as F
    B = 3
    p = F.dint_problem(oracle, B, np.zeros((B, 4)), N=11, tf=1.0)
    got = _recorded(p)
    v = np.array([0.6, 0.85, 0.7]); up = np.array([[1.0, 1.5], [0.8, 1.6], [1.2, 1.2]]); dn = -np.array([[0.9, 1.4], [1.6, 0.8], [1.2, 1.2]])
    x_max = np.full((B, 4), np.inf); x_max[:, 3] = v
    T.set_bounds_batch(p, 0, x_max=x_max, u_max=up, u_min=dn)
    (name, cid, flat), = got
    assert name == "set_constraint_limits_batch" and cid == 0
    np.testing.assert_array_equal(flat.reshape(B, 6), np.c_[v, up, np.full(B, -0.5), dn])      # [x4 max, u max, x1 min (the constraint's own), u min]
    # the finiteness pattern is the constraint's: a bound that appears or disappears for one trajectory would change p
    bad = x_max.copy(); bad[1, 0] = 2.0
    with pytest.raises(T.ArgumentError, match="entry 1 of .x; u. is finite for trajectory 1"):
        T.set_bounds_batch(p, 0, x_max=bad)
    bad = up.copy(); bad[2, 1] = np.inf
    with pytest.raises(T.ArgumentError, match="entry 6 of .x; u. is infinite for trajectory 2"):
        T.set_bounds_batch(p, 0, u_max=bad)
    with pytest.raises(T.DimensionMismatch):
        T.set_bounds_batch(p, 0, u_max=np.ones((B, 3)))
    with pytest.raises(T.ArgumentError, match="not a BoundConstraint"):
        T.set_bounds_batch(p, 1, u_max=up)
    with pytest.raises(T.DimensionMismatch):
        T.set_constraint_limits_batch(p, 0, np.zeros((B, 5)))
    assert len(got) == 1
    # StateBound / ControlBound / IndexedConstraint-wrapped bounds lower to the same kind: the verb works on them by id
    cons = T.ConstraintList(4, 2, 11)
    T.add_constraint(cons, T.ControlBound(4, 2, u_max=[1.0, 2.0], u_min=[-1.0, -2.0]), (1, 10))
    T.add_constraint(cons, T.IndexedConstraint(4, 2, T.BoundConstraint(2, 1, x_max=[0.5, np.inf], u_min=[-3.0]), ix=(3, 4), iu=(2, 2)), (1, 10))
    T.add_constraint(cons, T.NormConstraint(4, 2, 5.0, T.SecondOrderCone(), "control"), (1, 10))
    q = T.Problem(T.DoubleIntegrator(1.0, 2), p.obj, np.zeros(4), 1.0, constraints=cons, batch=B, lib=oracle)
    got = _recorded(q)
    T.set_bounds_batch(q, 0, u_max=np.tile([1.5, 2.5], (B, 1)))
    T.set_bounds_batch(q, 1, x_max=np.c_[np.full((B, 2), np.inf), [0.4, 0.5, 0.6], np.full(B, np.inf)])
    T.set_constraint_limits_batch(q, 2, [4.0, 5.0, 6.0])
    np.testing.assert_array_equal(got[0][2].reshape(B, 4), np.tile([1.5, 2.5, -1.0, -2.0], (B, 1)))
    np.testing.assert_array_equal(got[1][2].reshape(B, 2), np.c_[[0.4, 0.5, 0.6], np.full(B, -3.0)])   # x3 max (inner x1), u2 min (inner u1)
    np.testing.assert_array_equal(got[2][2], [4.0, 5.0, 6.0])
