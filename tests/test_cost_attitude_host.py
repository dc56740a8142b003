"""Per-trajectory attitude references (to_set_cost_attitude_batch / to_get_... / to_clear_... / to_set_tracking_attitude), everything that
needs no GPU: every refusal with its error class and message, the image of DevProblem::ga and its tiling (B = 70, the spare tile), the rules
by which ga rides on gw (csrc/path_plan.h cost_lane_step: what gw holds, which routing results and which tracking / weights refusals fire
after every step of every sequence) and k_track_lower compiled for the host (attitude rows exact copies of the right reference knot, none
with the mode off, the linear rows bit for bit the documented recipe in both modes) — all through tests/host_shim/attitude_harness.cpp, a
program of its own, also built with AddressSanitizer + UndefinedBehaviorSanitizer —, then the ctypes / ABI / Julia mirrors and the argument
checks of the Python verbs against a recording fake library."""
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
NAMES = ("set_cost_attitude_batch", "get_cost_attitude_batch", "clear_cost_attitude_batch", "set_tracking_attitude", "get_tracking_attitude")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _harness(tmp_path, flags=()):
    exe = tmp_path / "attitude_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", *flags, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "attitude_harness.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-3000:], r.stderr[-1500:])
    return r.stdout


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    return _harness(tmp_path_factory.mktemp("cost_attitude"))


def test_harness_under_asan_ubsan(tmp_path):
    out = _harness(tmp_path, SAN)
    assert int(out.split()[out.split().index("checks") + 1]) > 10 ** 6


def test_refusals_class_and_message(harness_out):
    cases = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"^case (\w+) code (-?\d+) msg (.*)$", harness_out, flags=re.M)}
    share = "TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, TO_MODEL_VECTOR and TO_MODEL_INFEASIBLE share their weights"
    only = "a per-trajectory attitude reference is the q_ref of a DiagonalQuatCost only"
    flight = "asynchronous solve is in flight"
    want = {
        "null_handle": (capi.TO_ERR_NULL, "null handle"), "null_handle_get": (capi.TO_ERR_NULL, "null handle"), "null_handle_clear": (capi.TO_ERR_NULL, "null handle"),
        "null_handle_track": (capi.TO_ERR_NULL, "null handle"),
        "null_q_ref": (capi.TO_ERR_NULL, "to_set_cost_attitude_batch: q_ref is NULL"), "null_q_ref_get": (capi.TO_ERR_NULL, "to_get_cost_attitude_batch: q_ref is NULL"),
        "id_low": (capi.TO_ERR_ARGUMENT, "cost id out of range"), "id_high": (capi.TO_ERR_ARGUMENT, "cost id out of range"),
        "id_high_get": (capi.TO_ERR_ARGUMENT, "cost id out of range"),
        "in_flight": (capi.TO_ERR_ARGUMENT, flight), "in_flight_get": (capi.TO_ERR_ARGUMENT, flight), "in_flight_clear": (capi.TO_ERR_ARGUMENT, flight),
        "nan": (capi.TO_ERR_ARGUMENT, "q_ref[2] of trajectory 37 is not finite"),      # the FIRST offender (trajectory 50 carries an infinity)
        "inf": (capi.TO_ERR_ARGUMENT, "q_ref[1] of trajectory 50 is not finite"),
        "diagonal": (capi.TO_ERR_UNSUPPORTED, "cost 0 is of kind DiagonalCost; " + only), "diagonal_get": (capi.TO_ERR_UNSUPPORTED, "cost 0 is of kind DiagonalCost; " + only),
        "quadratic": (capi.TO_ERR_UNSUPPORTED, "cost 0 is of kind QuadraticCost; " + only),
        "error_quadratic": (capi.TO_ERR_UNSUPPORTED, "cost 0 is of kind ErrorQuadratic; " + only + " (an ErrorQuadratic keeps its reference in its q slot)"),
        "model_7": (capi.TO_ERR_UNSUPPORTED, "hybrid double integrator (" + share), "model_8": (capi.TO_ERR_UNSUPPORTED, "model vector (" + share),
        "model_9": (capi.TO_ERR_UNSUPPORTED, "InfeasibleModel (double integrator, D = 1) (" + share),
        "model_11": (capi.TO_ERR_UNSUPPORTED, "InfeasibleModel (Cartpole) (" + share), "model_8_clear": (capi.TO_ERR_UNSUPPORTED, "model vector (" + share),
        "track_no_reference": (capi.TO_ERR_ARGUMENT, "to_set_tracking_attitude: no tracking reference is set"),
        "track_bad_flag": (capi.TO_ERR_ARGUMENT, "on must be 0 or 1; got 2"), "track_in_flight": (capi.TO_ERR_ARGUMENT, flight),
        "track_no_quat": (capi.TO_ERR_UNSUPPORTED, "none of the tracked costs is a DiagonalQuatCost"),
    }
    assert set(cases) == set(want)
    for k, (code, text) in want.items():
        assert cases[k][0] == code and text in cases[k][1], (k, cases[k])
    # every refusal is decided before any device call: the entry points validate first
    lib = (CSRC / "trajopt_hip.hip").read_text()
    body = lib[lib.index("int to_set_cost_attitude_batch("):lib.index("int to_get_cost_attitude_batch(")]
    assert body.index("validate_cost_attitude(") < body.index("use_device(") < body.index("upload_vec(")
    body = lib[lib.index("int to_set_tracking_attitude("):lib.index("int to_get_tracking_attitude(")]
    assert body.index("validate_tracking_attitude(") < body.index("use_device(")
    # ... and each is written into the header comment
    doc = HEADER[HEADER.index("One ATTITUDE REFERENCE per TRAJECTORY"):HEADER.index("int to_set_cost_attitude_batch(")]
    for word in ("TO_ERR_NULL", "TO_ERR_ARGUMENT", "TO_ERR_UNSUPPORTED", "not finite", "solve in flight", "TO_COST_DIAGONAL_QUAT", "ErrorQuadratic"):
        assert word in doc, word


def test_state_machine_rides_on_gw(harness_out):
    """After every step: gw holds the caller's weights exactly while the caller set some, the descriptors' diagonals while only attitudes keep
    the arrays alive, nothing once the last reason is gone (the harness asserts routing and refusals; here the printed states are read).
    The transitions come from the library's cost_lane_step; "what the arrays hold" comes from the harness's Model, a restatement of the
    library's cost_lane_apply, not the library itself — tests/test_gpu_cost_attitude.py::test_setter_semantics reads the device arrays."""
    states = {}
    for m in re.finditer(r"^state (\w+) step (\d+) weights (\d) attitude (\d) track (\d) routed (\d) gw (\d) ga (\d)$", harness_out, flags=re.M):
        states.setdefault(m.group(1), []).append(tuple(int(x) for x in m.groups()[2:]))
    NONE, DESC, CALLER = 0, 1, 2
    # set attitude, set weights, clear weights, clear attitude: (weights, attitude, track, routed, gw, ga)
    assert states["attitude_then_weights"] == [(0, 0, 0, 0, NONE, NONE), (0, 1, 0, 1, DESC, CALLER), (1, 1, 0, 1, CALLER, CALLER), (0, 1, 0, 1, DESC, CALLER),
                                               (0, 0, 0, 0, NONE, NONE)]
    assert states["weights_then_attitude"] == [(0, 0, 0, 0, NONE, NONE), (1, 0, 0, 1, CALLER, DESC), (1, 1, 0, 1, CALLER, CALLER), (1, 0, 0, 1, CALLER, DESC),
                                               (0, 0, 0, 0, NONE, NONE)]
    assert states["tracking"] == [(0, 0, 0, 0, NONE, NONE), (0, 0, 1, 1, DESC, CALLER), (0, 0, 0, 0, NONE, NONE)]
    assert len(states) == 9 and all(s[-1] == (0, 0, 0, 0, NONE, NONE) for s in states.values())
    plan = (CSRC / "path_plan.h").read_text()
    assert "struct CostLaneState" in plan and "cost_lane_step" in (CSRC / "trajopt_hip.hip").read_text()
    # the tracking refusal looks at the caller's flag, not at the pointer
    lib = (CSRC / "trajopt_hip.hip").read_text()
    facts = lib[lib.index("static TrackFacts track_facts("):lib.index("static int track_lower(")]
    assert "h->lane.weights" in facts and "P.gw != nullptr" not in facts


def test_ctypes_signatures_and_abi_symbols():
    C = capi.C
    assert capi.HIP_ONLY["set_cost_attitude_batch"] == [capi._H, C.c_int32, capi._PD]
    assert capi.HIP_ONLY["get_cost_attitude_batch"] == [capi._H, C.c_int32, capi._PD]
    assert capi.HIP_ONLY["clear_cost_attitude_batch"] == [capi._H]
    assert capi.HIP_ONLY["set_tracking_attitude"] == [capi._H, C.c_int32]
    assert capi.HIP_ONLY["get_tracking_attitude"] == [capi._H, capi._PI]
    for n in NAMES:
        assert n in capi.OPTIONAL_HIP and n not in capi.SIGNATURES      # found by symbol lookup; the oracle does not have them
        assert re.search(r"^int to_" + n + r"\(to_handle\* h", HEADER, flags=re.M), n
        assert n in api.__all__ and callable(getattr(T, n))
    assert "#define TO_ABI_VERSION 7\n" in HEADER and "#define TO_ABI_MINOR 1\n" in HEADER and capi.TO_ABI_VERSION == 7
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    assert "to_set_cost_attitude_batch" in history and "to_set_tracking_attitude" in history and history.rstrip().endswith("*/")
    # the two sentences that said "shared" now point at the new calls
    assert "to_set_cost_attitude_batch below gives each trajectory its own" in HEADER and "to_set_tracking_attitude below is turned on" in HEADER
    lib = CSRC / "libtrajopt_hip.so"
    if lib.exists():  # a built tree exports them (the build itself binds every name the library has)
        syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(r"\bT to_" + n + r"$", syms, flags=re.M), n


def test_julia_shim_binds_the_verbs():
    shim = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
    for verb, sym, types in (("set_cost_attitude_batch!", "to_set_cost_attitude_batch", "(Ptr{Cvoid}, Int32, Ptr{Float64})"),
                             ("cost_attitude_batch", "to_get_cost_attitude_batch", "(Ptr{Cvoid}, Int32, Ptr{Float64})"),
                             ("clear_cost_attitude_batch!", "to_clear_cost_attitude_batch", "(Ptr{Cvoid},)"),
                             ("set_tracking_attitude!", "to_set_tracking_attitude", "(Ptr{Cvoid}, Int32)")):
        assert f"function {verb}(" in shim and f"ccall((:{sym}, lib), Cint, {types}" in shim, verb
        assert re.search(r"^export .*\b" + re.escape(verb), shim, flags=re.M), verb
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_set_cost_attitude_batch; throw_error = false)" in shim
    assert re.search(r"function TO\.set_goal_state!\(p::BatchProblem, Xf::Matrix\{Float64\}[^)]*attitude::Bool = false", shim)
    assert 'size(q_ref) == (4, p.B) || throw(DimensionMismatch' in shim      # the size check stands before the ccall


def test_the_oracle_refuses_per_trajectory_attitudes(oracle):
    p = configs.quadrotor_problem(batch=3, N=11, lib=oracle)
    Xf = np.tile(p.xf, (3, 1))
    for call in (lambda: T.set_cost_attitude_batch(p, 0, np.ones((3, 4))), lambda: T.get_cost_attitude_batch(p, 0), lambda: T.clear_cost_attitude_batch(p),
                 lambda: T.set_tracking_attitude(p, True), lambda: T.get_tracking_attitude(p), lambda: T.set_goal_state(p, Xf, attitude=True)):
        with pytest.raises(T.UnsupportedError, match="per-trajectory attitude references need a HIP library"):
            call()
    T.set_goal_state(p, Xf)                                                   # the default keeps today's call, on the oracle too


class _Recorder:
    """Stands in for the library behind a problem (found by symbol lookup: the names are in ``_fn``); records what the verbs hand to it."""

    def __init__(self):
        self._fn = dict.fromkeys(NAMES + ("set_cost_linear_batch", "set_tracking_reference_batch", "set_tracking_window"))


def _recorded(prob):
    prob._lib = _Recorder()
    got = []

    def call(name, *args):
        if name == "set_cost_attitude_batch":
            got.append((name, args[0], np.ctypeslib.as_array(args[1], shape=(prob.B, 4)).copy()))
        elif name == "set_cost_linear_batch":
            got.append((name, args[0], np.ctypeslib.as_array(args[1], shape=(prob.B, prob.n)).copy()))
        else:
            got.append((name,) + tuple(a for a in args if isinstance(a, int)))
    prob._call = call
    return got


def test_python_verbs_check_shapes_and_pass_contiguous_rows(oracle):
    B = 3
    p = configs.quadrotor_problem(batch=B, N=11, lib=oracle)
    got = _recorded(p)
    A = np.arange(12.0).reshape(B, 4) + 1.0
    T.set_cost_attitude_batch(p, 1, A[:, ::-1])                 # a strided view goes out contiguous
    assert got[0][:2] == ("set_cost_attitude_batch", 1)
    np.testing.assert_array_equal(got[0][2], A[:, ::-1])
    for bad in (np.ones((B, 3)), np.ones((4, B)), np.ones(4), np.ones((B + 1, 4))):
        with pytest.raises(T.DimensionMismatch, match=r"q_ref must be \[B, 4\]"):
            T.set_cost_attitude_batch(p, 0, bad)
    assert len(got) == 1                                        # a refused call hands nothing to the library
    T.set_tracking_attitude(p, True); T.set_tracking_attitude(p, False)
    assert got[1:] == [("set_tracking_attitude", 1), ("set_tracking_attitude", 0)]


def test_set_goal_state_attitude_keyword(oracle):
    """attitude=True: every DiagonalQuatCost gets q_ref_b = Xf[b, q_ind - 1] next to q_b = -Q xf_b; the default keeps today's calls; a 1-D xf
    with attitude=True raises; so does a problem without a DiagonalQuatCost; clear_goal_state_batch clears what was set that way."""
    B = 3
    p = configs.quadrotor_problem(batch=B, N=11, lib=oracle)    # costs: 0 stage, 1 terminal, both QuatLQRCost
    got = _recorded(p)
    rng = np.random.default_rng(5)
    Xf = rng.uniform(-1, 1, (B, 13))
    T.set_goal_state(p, Xf)
    assert [g[0] for g in got] == ["set_cost_linear_batch"] * 2 and not getattr(p, "_goal_attitude", False)
    del got[:]
    T.set_goal_state(p, Xf, attitude=True)
    # the attitudes go first: the library's own refusals (a model without per-trajectory cost data) then come before any other change
    assert [(g[0], g[1]) for g in got] == [("set_cost_attitude_batch", 0), ("set_cost_attitude_batch", 1), ("set_cost_linear_batch", 0), ("set_cost_linear_batch", 1)]
    for g in got[:2]:
        np.testing.assert_array_equal(g[2], Xf[:, 3:7])         # used as given: not normalised
    np.testing.assert_array_equal(got[2][2], -p._cost_objs[0].Q * Xf)
    del got[:]
    Xb = Xf.copy(); Xb[1, 9] = np.inf; Xb[2, 4] = np.nan
    with pytest.raises(T.ArgumentError, match=r"Xf\[1, 9\] is not finite"):
        T.set_goal_state(p, Xb, attitude=True)
    assert got == []                                            # refused before anything changes
    del got[:]
    T.clear_goal_state_batch(p)
    assert [g[0] for g in got] == ["clear_cost_linear_batch", "clear_constraint_params_batch", "clear_cost_attitude_batch"]
    del got[:]
    T.clear_goal_state_batch(p)                                  # nothing set that way any more: today's two calls
    assert [g[0] for g in got] == ["clear_cost_linear_batch", "clear_constraint_params_batch"]
    del got[:]
    with pytest.raises(T.ArgumentError, match="attitude=True needs one goal per trajectory"):
        T.set_goal_state(p, Xf[0], attitude=True)
    with pytest.raises(T.DimensionMismatch):
        T.set_goal_state(p, Xf[:, :12], attitude=True)
    # a q_ind of its own is followed
    p._cost_objs[1].q_ind = (7, 4, 13, 1)
    T.set_goal_state(p, Xf, attitude=True)
    np.testing.assert_array_equal(got[1][2], Xf[:, [6, 3, 12, 0]])
    assert len(got) == 4
    # no DiagonalQuatCost: refused before anything is handed over
    c = configs.cartpole_problem(batch=B, N=11, tf=0.5, lib=oracle)
    gc = _recorded(c)
    with pytest.raises(T.ArgumentError, match="no DiagonalQuatCost"):
        T.set_goal_state(c, np.zeros((B, 4)), attitude=True)
    assert gc == []


def test_set_tracking_reference_batch_attitude_keyword(oracle):
    import attitude_fleets as AF
    f = AF.tracking(3)
    p = f.problem(oracle)
    got = _recorded(p)
    T.set_tracking_reference_batch(p, f.Xref, f.Uref, start=f.start, end="hold")
    assert [g[0] for g in got] == ["set_tracking_reference_batch"]
    del got[:]
    T.set_tracking_reference_batch(p, f.Xref, f.Uref, start=f.start, end="hold", attitude=True)
    assert [g[0] for g in got] == ["set_tracking_reference_batch", "set_tracking_attitude"] and got[1][1] == 1
