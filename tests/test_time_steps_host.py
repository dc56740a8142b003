"""Per-trajectory time steps (to_set_time_steps_batch / to_get_... / to_clear_...), everything that needs no GPU: the host-only lowering
dt[(N-1), B] -> the tiled array DevProblem::dtb with every refusal (csrc/desc_lower.h lower_time_steps, compiled as a program of its own —
also under AddressSanitizer + UndefinedBehaviorSanitizer), the routing of a flagged handle (csrc/path_plan.h), the ctypes / ABI / Julia
mirrors, and the argument checks of the Python verbs."""
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
NAMES = ("set_time_steps_batch", "get_time_steps_batch", "clear_time_steps_batch")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _harness(tmp_path, flags=()):
    exe = tmp_path / "time_steps_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "time_steps_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-3000:], r.stderr[-1500:])
    return r.stdout


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    return _harness(tmp_path_factory.mktemp("steps"))


def test_lowering_harness_under_asan_ubsan(tmp_path):
    """Tiling (padding lanes of the last tile and the spare tile on the shared steps), the round trip and the refusals, as a stand-alone
    program built with the sanitizers."""
    _harness(tmp_path, SAN)


def test_refusals_class_and_message(harness_out):
    cases = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"^case (\w+) code (-?\d+) msg (.*)$", harness_out, flags=re.M)}
    want = {
        "nan": (capi.TO_ERR_ARGUMENT, "time step 1 of trajectory 1 is not finite"),
        "inf": (capi.TO_ERR_ARGUMENT, "time step 2 of trajectory 2 is not finite"),
        "zero": (capi.TO_ERR_ARGUMENT, "time step 2 of trajectory 0 is not > 0"),
        "negative": (capi.TO_ERR_ARGUMENT, "time step 0 of trajectory 2 is not > 0"),
        "first_of_two": (capi.TO_ERR_ARGUMENT, "time step 2 of trajectory 1 is not > 0"),     # the FIRST offending trajectory and knot
        "fine": (capi.TO_OK, ""),
    }
    assert set(cases) == set(want)
    for k, (code, text) in want.items():
        assert cases[k][0] == code and text in cases[k][1], (k, cases[k])
    assert capi._ERRORS[capi.TO_ERR_ARGUMENT] is T.ArgumentError and capi._ERRORS[capi.TO_ERR_UNSUPPORTED] is T.UnsupportedError


def test_a_flagged_handle_plans_what_plants_plans(tmp_path):
    exe = tmp_path / "time_steps_plan_harness"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", str(CSRC), str(SHIM / "time_steps_plan_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    words = r.stdout.split()
    count = lambda k: int(words[words.index(k) + 1])
    assert count("fails") == 0 and count("checks") > 4 * 10 ** 5
    # every kind of handle was reached: lane and MFMA layouts, compaction kept (MFMA) and dropped
    for k in ("steps", "reports", "lane_handles", "mfma_handles", "compact_kept", "compact_dropped"):
        assert count(k) > 1000, (k, r.stdout)
    assert count("variants") == 32
    # the library derives its routing from these predicates, not from a copy
    src = (CSRC / "trajopt_hip.hip").read_text()
    assert "routed_as_plants(h->a.P.pm != nullptr, h->a.P.dtb != nullptr)" in src and "tf.time_steps = P.dtb != nullptr" in src


def test_ctypes_signatures_and_abi_symbols():
    assert capi.HIP_ONLY["set_time_steps_batch"] == [capi._H, capi._PD]
    assert capi.HIP_ONLY["get_time_steps_batch"] == [capi._H, capi._PD]
    assert capi.HIP_ONLY["clear_time_steps_batch"] == [capi._H]
    for n in NAMES:
        assert n in capi.OPTIONAL_HIP and n not in capi.SIGNATURES      # found by symbol lookup; the oracle does not have them
        assert re.search(r"^int to_" + n + r"\(to_handle\* h", HEADER, flags=re.M), n
    assert "#define TO_ABI_VERSION 7\n" in HEADER and "#define TO_ABI_MINOR 1\n" in HEADER and capi.TO_ABI_VERSION == 7
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    assert "to_set_time_steps_batch" in history and "symbol lookup" in history
    for n in ("set_time_steps_batch", "set_final_times_batch", "time_steps", "clear_time_steps_batch"):
        assert n in api.__all__ and callable(getattr(T, n))
    lib = CSRC / "libtrajopt_hip.so"
    if lib.exists():  # a built tree exports them (the build itself binds every name the library has)
        syms = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(r"\bT to_" + n + r"$", syms, flags=re.M), n


def test_julia_shim_binds_the_verbs():
    shim = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
    for verb, sym, types in (("set_time_steps_batch!", "to_set_time_steps_batch", "(Ptr{Cvoid}, Ptr{Float64})"),
                             ("time_steps_batch", "to_get_time_steps_batch", "(Ptr{Cvoid}, Ptr{Float64})"),
                             ("clear_time_steps_batch!", "to_clear_time_steps_batch", "(Ptr{Cvoid},)")):
        assert f"function {verb}(" in shim and f"ccall((:{sym}, lib), Cint, {types}" in shim, verb
        assert re.search(r"^export .*\b" + re.escape(verb), shim, flags=re.M), verb
    assert "function set_final_times_batch!(" in shim and re.search(r"^export .*\bset_final_times_batch!", shim, flags=re.M)
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_set_time_steps_batch; throw_error = false)" in shim
    # each verb that takes or returns the steps checks size(...) == (N-1, B) and throws DimensionMismatch
    for verb, end in (("set_time_steps_batch!", "function set_final_times_batch!"), ("set_final_times_batch!", "function time_steps_batch"),
                      ("time_steps_batch", "function clear_time_steps_batch!")):
        body = shim[shim.index(f"function {verb}("):shim.index(end)]
        assert "== (p.N - 1, p.B) || throw(DimensionMismatch(" in body, verb
    # the uniform step of set_final_times_batch!: Problem's own expression
    assert "(tf[b] - TO.get_initial_time(p.prob)) / (p.N - 1)" in shim


def test_the_oracle_refuses_per_trajectory_steps(oracle):
    import model_params_fleet as M
    p = M.build("cartpole", oracle, 3, N=11, tf=0.5)
    for call in (lambda: T.set_time_steps_batch(p, np.full((3, 10), 0.05)), lambda: T.set_final_times_batch(p, np.ones(3)),
                 lambda: T.time_steps(p), lambda: T.clear_time_steps_batch(p)):
        with pytest.raises(T.UnsupportedError, match="to_set_time_steps_batch"):
            call()


def test_python_verbs_check_shapes_and_form_the_uniform_step(oracle):
    import model_params_fleet as M
    B, N = 3, 11
    p = M.build("cartpole", oracle, B, N=N, tf=0.5)
    got = []
    p._lib = type("Rec", (), {"_fn": dict.fromkeys(NAMES)})()     # stands in for a library that has the symbols
    p._call = lambda name, *args: got.append((name, np.ctypeslib.as_array(args[0], shape=(B * (N - 1),)).copy() if args else None))
    tf = np.array([0.5, 0.43, 0.61])
    T.set_final_times_batch(p, tf)
    (name, flat), = got
    assert name == "set_time_steps_batch"
    h = flat.reshape(B, N - 1)                                     # trajectory-major, knot fastest: [(N-1)*B] of the C-ABI
    for b in range(B):
        assert np.all(h[b] == (tf[b] - p.t0) / (N - 1))            # bit for bit what Problem(tf=tf[b]) forms
    dt = np.random.default_rng(0).uniform(0.01, 0.1, (B, N - 1))
    T.set_time_steps_batch(p, dt)
    np.testing.assert_array_equal(got[1][1].reshape(B, N - 1), dt)
    for bad in (np.ones((B, N)), np.ones((N - 1, B)), np.ones(B * (N - 1)), np.ones((B + 1, N - 1))):
        with pytest.raises(T.DimensionMismatch):
            T.set_time_steps_batch(p, bad)
    for bad in (np.ones(B + 1), np.ones((B, 1)), 1.0):
        with pytest.raises(T.DimensionMismatch):
            T.set_final_times_batch(p, bad)
    assert len(got) == 2
