"""Per-trajectory cost weights (to_set_cost_weights_batch / to_get_... / to_clear_...), everything that needs no GPU: every refusal with its
error class, the host copy behind DevProblem::gw and its tiling, the routing of a handle with weights (csrc/path_plan.h TableFlags::
cost_weights: what a con_limits handle plans, without the preloaded stage cost; without the flag: what it plans today) and the re-use rule of
the repacked working set — all through tests/host_shim/cost_weights_harness.cpp, a program of its own, also built with AddressSanitizer +
UndefinedBehaviorSanitizer —, the ctypes / ABI / Julia mirrors, the argument checks of the Python verbs against a recording fake library, and
q_b = -Q_b xf_b from set_LQR_weights_batch."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import capi
from trajectoryoptimization_jl_amd import api, configs

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
SHIM = ROOT / "tests" / "host_shim"
HEADER = (ROOT / "include" / "trajopt_hip.h").read_text()
NAMES = ("set_cost_weights_batch", "get_cost_weights_batch", "clear_cost_weights_batch")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _harness(tmp_path, flags=()):
    exe = tmp_path / "cost_weights_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "cost_weights_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-3000:], r.stderr[-1500:])
    return r.stdout


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    return _harness(tmp_path_factory.mktemp("cost_weights"))


def test_harness_under_asan_ubsan(tmp_path):
    _harness(tmp_path, SAN)


def test_refusals_class_and_message(harness_out):
    cases = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"^case (\w+) code (-?\d+) msg (.*)$", harness_out, flags=re.M)}
    share = "TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, TO_MODEL_VECTOR and TO_MODEL_INFEASIBLE share their weights"
    want = {
        "null_handle": (capi.TO_ERR_NULL, "null handle"), "null_handle_get": (capi.TO_ERR_NULL, "null handle"), "null_handle_clear": (capi.TO_ERR_NULL, "null handle"),
        "id_low": (capi.TO_ERR_ARGUMENT, "cost id out of range"), "id_high": (capi.TO_ERR_ARGUMENT, "cost id out of range"),
        "id_high_get": (capi.TO_ERR_ARGUMENT, "cost id out of range"),
        "both_null": (capi.TO_ERR_ARGUMENT, "Q and R are both NULL"), "both_null_get": (capi.TO_ERR_ARGUMENT, "Q and R are both NULL"),
        "in_flight": (capi.TO_ERR_ARGUMENT, "asynchronous solve is in flight"), "in_flight_clear": (capi.TO_ERR_ARGUMENT, "asynchronous solve is in flight"),
        "nan_Q": (capi.TO_ERR_ARGUMENT, "Q[2] of trajectory 37 is not finite"),        # the FIRST offender (trajectory 50 carries an infinity)
        "inf_R": (capi.TO_ERR_ARGUMENT, "R[1] of trajectory 69 is not finite"),
        "quadratic": (capi.TO_ERR_UNSUPPORTED, "cost 2 is of kind QuadraticCost"), "error_quadratic": (capi.TO_ERR_UNSUPPORTED, "cost 2 is of kind ErrorQuadratic"),
        "quadratic_get": (capi.TO_ERR_UNSUPPORTED, "cost 2 is of kind QuadraticCost"),
        "model_7": (capi.TO_ERR_UNSUPPORTED, "hybrid double integrator (" + share), "model_8": (capi.TO_ERR_UNSUPPORTED, "model vector (" + share),
        "model_9": (capi.TO_ERR_UNSUPPORTED, "InfeasibleModel (double integrator, D = 1) (" + share),
        "model_11": (capi.TO_ERR_UNSUPPORTED, "InfeasibleModel (Cartpole) (" + share), "model_8_clear": (capi.TO_ERR_UNSUPPORTED, "model vector (" + share),
        "tracking_first": (capi.TO_ERR_UNSUPPORTED, "the handle holds a tracking reference"),
        "weights_first": (capi.TO_ERR_UNSUPPORTED, "to_set_tracking_reference_batch: the handle carries per-trajectory cost weights"),
    }
    assert set(cases) == set(want)
    for k, (code, text) in want.items():
        assert cases[k][0] == code and text in cases[k][1], (k, cases[k])
    assert capi._ERRORS[capi.TO_ERR_ARGUMENT] is T.ArgumentError and capi._ERRORS[capi.TO_ERR_UNSUPPORTED] is T.UnsupportedError
    # the values are held to being finite and to nothing else; the reference's definiteness warning is cited where that is decided
    src = (CSRC / "desc_lower.h").read_text()
    assert "src/cost_functions.jl:337-343" in src
    # every refusal is decided before any device call: the entry points validate first
    lib = (CSRC / "trajopt_hip.hip").read_text()
    body = lib[lib.index("int to_set_cost_weights_batch("):lib.index("int to_get_cost_weights_batch(")]
    assert body.index("validate_cost_weights(") < body.index("use_device(") < body.index("cost_weights_store(")


def test_routing_and_repack_rule(harness_out):
    words = harness_out.split()
    count = lambda k: int(words[words.index(k) + 1])
    assert count("fails") == 0 and count("checks") > 10 ** 6
    # both sides were reached: unflagged handles on the fused cooperative / scan kernels and on preloaded stage costs; flagged ones on the fused
    # lane path, in two-wave workgroups and with a repacked working set in the report
    for k in ("flagged", "plain", "fused_plain", "simple_plain", "lane_flagged", "two_wave_flagged", "repack_flagged"):
        assert count(k) > 1000, (k, harness_out[-600:])
    plan = (CSRC / "path_plan.h").read_text()
    assert re.search(r"bool cost_weights = false;", plan) and "bool cost_weights /* gw */ = false" in plan   # a defaulted field, trailing defaulted arguments


def test_ctypes_signatures_and_abi_symbols():
    C = capi.C
    assert capi.HIP_ONLY["set_cost_weights_batch"] == [capi._H, C.c_int32, capi._PD, capi._PD]
    assert capi.HIP_ONLY["get_cost_weights_batch"] == [capi._H, C.c_int32, capi._PD, capi._PD]
    assert capi.HIP_ONLY["clear_cost_weights_batch"] == [capi._H]
    for n in NAMES:
        assert n in capi.OPTIONAL_HIP and n not in capi.SIGNATURES      # found by symbol lookup; the oracle does not have them
        assert re.search(r"^int to_" + n + r"\(to_handle\* h", HEADER, flags=re.M), n
    assert "#define TO_ABI_VERSION 7\n" in HEADER and "#define TO_ABI_MINOR 1\n" in HEADER and capi.TO_ABI_VERSION == 7
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    assert "to_set_cost_weights_batch" in history and history.rstrip().endswith("*/")
    for n in NAMES + ("set_LQR_weights_batch",):
        assert n in api.__all__ and callable(getattr(T, n))
    lib = CSRC / "libtrajopt_hip.so"
    if lib.exists():  # a built tree exports them (the build itself binds every name the library has)
        syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(r"\bT to_" + n + r"$", syms, flags=re.M), n


def test_julia_shim_binds_the_verbs():
    shim = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
    for verb, sym, types in (("set_cost_weights_batch!", "to_set_cost_weights_batch", "(Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64})"),
                             ("cost_weights_batch", "to_get_cost_weights_batch", "(Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64})"),
                             ("clear_cost_weights_batch!", "to_clear_cost_weights_batch", "(Ptr{Cvoid},)")):
        assert f"function {verb}(" in shim and f"ccall((:{sym}, lib), Cint, {types}" in shim, verb
        assert re.search(r"^export .*\b" + re.escape(verb), shim, flags=re.M), verb
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_set_cost_weights_batch; throw_error = false)" in shim


def test_the_oracle_refuses_per_trajectory_weights(oracle):
    p = configs.cartpole_problem(batch=3, N=11, tf=0.5, lib=oracle)
    for call in (lambda: T.set_cost_weights_batch(p, 0, Q=np.ones((3, 4))), lambda: T.get_cost_weights_batch(p, 0), lambda: T.clear_cost_weights_batch(p),
                 lambda: T.set_LQR_weights_batch(p, np.ones((3, 4)), np.ones((3, 1)))):
        with pytest.raises(T.UnsupportedError, match="to_set_cost_weights_batch"):
            call()


class _Recorder:
    """Stands in for the library behind a problem (found by symbol lookup: the names are in ``_fn``); records what the verbs hand to it."""

    def __init__(self):
        self._fn = dict.fromkeys(NAMES + ("set_cost_linear_batch",))


def _recorded(prob):
    prob._lib = _Recorder()
    got = []

    def call(name, *args):
        n, m, B = prob.n, prob.m, prob.B
        arr = [None if a is None else np.ctypeslib.as_array(a, shape=(B, k)).copy() for a, k in zip(args[1:], (n, m))]
        got.append((name, args[0] if args else None, *arr))
    prob._call = call
    return got


def test_python_verbs_check_shapes_and_pass_contiguous_columns(oracle):
    B = 3
    p = configs.cartpole_problem(batch=B, N=11, tf=0.5, lib=oracle)
    got = _recorded(p)
    Q = np.arange(12.0).reshape(B, 4) + 1.0
    R = np.array([[0.5], [0.25], [2.0]])
    T.set_cost_weights_batch(p, 1, Q=Q[:, ::-1], R=R)           # a strided view goes out contiguous
    T.set_cost_weights_batch(p, 0, R=R)
    assert got[0][:2] == ("set_cost_weights_batch", 1) and got[1][:2] == ("set_cost_weights_batch", 0)
    np.testing.assert_array_equal(got[0][2], Q[:, ::-1]); np.testing.assert_array_equal(got[0][3], R)
    assert got[1][2] is None
    np.testing.assert_array_equal(got[1][3], R)
    for bad in (dict(Q=np.ones((B, 5))), dict(Q=np.ones((4, B))), dict(R=np.ones((B, 2))), dict(R=np.ones(B)), dict(Q=np.ones((B + 1, 4)))):
        with pytest.raises(T.DimensionMismatch, match=r"must be \[B, [nm]\]"):
            T.set_cost_weights_batch(p, 0, **bad)
    with pytest.raises(T.ArgumentError, match="give Q, R or both"):
        T.set_cost_weights_batch(p, 0)
    assert len(got) == 2                                        # a refused call hands nothing to the library


def test_set_LQR_weights_batch_sets_the_goal_terms_of_the_new_weights(oracle):
    """Stage costs get Q_b, R_b, the terminal cost Qf_b and R_b; with goals q_b = -Q_b xf_b, r_b = -R_b uf_b go through to_set_cost_linear_batch."""
    B = 3
    p = configs.cartpole_problem(batch=B, N=11, tf=0.5, lib=oracle)     # costs: 0 stage, 1 terminal; xf = [0, pi, 0, 0]
    got = _recorded(p)
    rng = np.random.default_rng(9)
    Q, R, Qf = rng.uniform(0.1, 1.0, (B, 4)), rng.uniform(0.1, 1.0, (B, 1)), rng.uniform(10.0, 100.0, (B, 4))
    T.set_LQR_weights_batch(p, Q, R, Qf)                                # goal: the problem's own xf
    assert [(g[0], g[1]) for g in got] == [("set_cost_weights_batch", 0), ("set_cost_linear_batch", 0), ("set_cost_weights_batch", 1), ("set_cost_linear_batch", 1)]
    np.testing.assert_array_equal(got[0][2], Q); np.testing.assert_array_equal(got[0][3], R)
    np.testing.assert_array_equal(got[2][2], Qf); np.testing.assert_array_equal(got[2][3], R)
    np.testing.assert_array_equal(got[1][2], -Q * p.xf); np.testing.assert_array_equal(got[1][3], np.zeros((B, 1)))
    np.testing.assert_array_equal(got[3][2], -Qf * p.xf)
    # one goal and one reference control per trajectory
    del got[:]
    Xf, Uf = rng.uniform(-1, 1, (B, 4)), rng.uniform(-1, 1, (B, 1))
    T.set_LQR_weights_batch(p, Q, R, Qf, xf=Xf, uf=Uf)
    np.testing.assert_array_equal(got[1][2], -Q * Xf); np.testing.assert_array_equal(got[1][3], -R * Uf)
    np.testing.assert_array_equal(got[3][2], -Qf * Xf); np.testing.assert_array_equal(got[3][3], -R * Uf)
    np.testing.assert_array_equal(p.xf_batch, Xf)
    # Qf left out: the terminal cost is not touched; the problem's per-trajectory goals (xf_batch) are the default goal
    del got[:]
    T.set_LQR_weights_batch(p, Q, R)
    assert [(g[0], g[1]) for g in got] == [("set_cost_weights_batch", 0), ("set_cost_linear_batch", 0)]
    np.testing.assert_array_equal(got[1][2], -Q * Xf)
    with pytest.raises(T.DimensionMismatch):
        T.set_LQR_weights_batch(p, Q[:, :3], R)
    with pytest.raises(T.ArgumentError, match="Q and R are both needed"):
        T.set_LQR_weights_batch(p, Q, None)
    assert "c`` stays the descriptor's" in T.set_LQR_weights_batch.__doc__
