"""Per-trajectory model parameters (to_set_model_params_batch / to_get_... / to_clear_...), everything that needs no GPU: the path logic
behind the trailing ``plants`` argument of csrc/path_plan.h compiled for the host (tests/host_shim/plants_plan_harness.cpp), the three
symbols in the header, the ctypes mirror, the Julia shim and the built library, TO_ABI_MINOR still 1, and the Python wrapper's refusals."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "trajopt_hip.h").read_text()
SHIM = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
NAMES = ("set_model_params_batch", "get_model_params_batch", "clear_model_params_batch")


def test_path_logic_with_per_trajectory_plants(tmp_path):
    """Flag set, whatever the shape (B = 1 .. 70 000, Cartpole / double integrator / Quadrotor traits, every knob): plan_step never returns
    STEP_SCAN, STEP_FUSED_COOP or STEP_FUSED_LANE, store_x == 1, no two-launch search, no two-wave workgroup, no repacked working set, and
    path_report shows info[1] == 0, info[5] == 0, (info[7] & 2) == 0.  Without the flag every result equals what the predicates returned
    before they had the argument (kept verbatim in the harness)."""
    exe = tmp_path / "plants_plan_harness"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", str(ROOT / "trajectoryoptimization.jl_amd" / "csrc"),
                    str(ROOT / "tests" / "host_shim" / "plants_plan_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-6000:]
    words = r.stdout.split()
    count = lambda k: int(words[words.index(k) + 1])
    assert count("fails") == 0 and count("checks") > 10 ** 6
    for k in ("flagged", "plain", "lane_handles", "mfma_handles", "compact_kept", "compact_dropped"):   # every kind of handle was reached
        assert count(k) > 1000, (k, r.stdout)


def test_the_existing_path_plan_harness_still_compiles_unchanged(tmp_path):
    """The trailing arguments are defaulted: tests/host_shim/path_plan_harness.cpp, which calls the predicates without them, compiles as is."""
    subprocess.run(["g++", "-std=c++17", "-O0", "-fsyntax-only", "-I", str(ROOT / "trajectoryoptimization.jl_amd" / "csrc"),
                    str(ROOT / "tests" / "host_shim" / "path_plan_harness.cpp")], check=True)


def test_symbols_in_header_mirror_shim_and_library():
    for name in NAMES:
        sym = "to_" + name
        assert re.search(r"^int\s+" + sym + r"\s*\(to_handle\* h", HEADER, flags=re.M), sym
        assert name in T.capi.HIP_ONLY and name in T.capi.OPTIONAL_HIP and name not in T.capi.SIGNATURES, sym
        assert f"ccall((:{sym}, lib), Cint," in SHIM, sym
    assert T.capi.HIP_ONLY["set_model_params_batch"] == T.capi.HIP_ONLY["get_model_params_batch"] == [C.c_void_p, C.POINTER(C.c_double)]
    assert T.capi.HIP_ONLY["clear_model_params_batch"] == [C.c_void_p]
    # hosts find them by symbol lookup: the shim looks before it calls, and checks the shape the advisor asked for on the batch setters
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_set_model_params_batch; throw_error = false)" in SHIM
    body = SHIM[SHIM.index("function set_model_params_batch!"):]
    body = body[: body.index("\nend")]
    assert "size(params) == (16, p.B) || throw(DimensionMismatch" in body and body.index("DimensionMismatch") < body.index("ccall")
    for verb in ("set_model_params_batch!", "model_params_batch", "clear_model_params_batch!"):
        assert re.search(r"^export .*\b" + re.escape(verb), SHIM, flags=re.M | re.S), verb
    lib = T.load_hip_library()
    dll = C.CDLL(lib.path)
    for name in NAMES:
        assert hasattr(dll, "to_" + name) and name in lib._fn, name


def test_abi_minor_did_not_move():
    """The three entry points are detected by symbol lookup, not announced by the minor version (the header's ABI history says so)."""
    assert re.search(r"^#define TO_ABI_MINOR 1$", HEADER, flags=re.M)
    assert T.capi.TO_ABI_MINOR == 1 and re.search(r"^const TO_ABI_MINOR = Int32\(1\)", SHIM, flags=re.M)
    assert T.load_hip_library().abi_minor() == 1
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    assert "to_set_model_params_batch" in history and "dlsym" in history and "WITHOUT raising TO_ABI_MINOR" in history


def test_a_library_without_the_symbols_still_binds(tmp_path):
    """Optional binding: a library that exports everything but the three new symbols loads; the wrappers then refuse."""
    class Old(T.capi.Library):
        def __init__(self):
            self._fn = {"rollout": None}
    class P:
        _lib, B, model = Old(), 3, T.Cartpole()
    for call in (lambda: T.set_model_params(P(), np.zeros((3, 16))), lambda: T.model_params(P()), lambda: T.clear_model_params(P())):
        with pytest.raises(T.UnsupportedError, match="to_set_model_params_batch"):
            call()


class _Recorder:
    """A problem whose library exports the entry points and records the calls (no GPU)."""
    _fn = dict.fromkeys(NAMES)

    def __init__(self, model, B):
        self._lib, self.model, self.B, self.calls = self, model, B, []

    def _call(self, name, *args):
        self.calls.append(name)

    @staticmethod
    def _pd(a):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == np.float64
        return a


def test_wrapper_refuses_bad_input_before_the_library_sees_it(oracle):
    p = _Recorder(T.Cartpole(), 4)
    with pytest.raises(T.DimensionMismatch, match=r"\[B=4, 16\]"):
        T.set_model_params(p, np.zeros((3, 16)))
    with pytest.raises(T.DimensionMismatch):
        T.set_model_params(p, np.zeros((4, 4)))
    with pytest.raises(T.DimensionMismatch):
        T.set_model_params(p, [T.Cartpole()] * 5)
    with pytest.raises(T.ArgumentError, match=r"models\[2\] must be a Cartpole"):
        T.set_model_params(p, [T.Cartpole(), T.Cartpole(), T.DoubleIntegrator(1.0, 2), T.Cartpole()])
    q = _Recorder(T.Quadrotor(), 2)
    with pytest.raises(T.ArgumentError, match=r"models\[1\] must be a Quadrotor with the problem's dimensions"):
        T.set_model_params(q, [T.Quadrotor(), T.Quadrotor(rotation="mrp")])
    bad = np.ones((4, 16)); bad[3, 2] = np.inf
    with pytest.raises(T.ArgumentError, match="trajectory 3 are not finite"):
        T.set_model_params(p, bad)
    with pytest.raises(T.ArgumentError, match="trajectory 1 are not finite"):
        T.set_model_params(p, [T.Cartpole(), T.Cartpole(mp=float("nan")), T.Cartpole(), T.Cartpole()])
    assert p.calls == [] and q.calls == []
    T.set_model_params(p, [T.Cartpole(mp=0.2 + 0.01 * b) for b in range(4)])
    T.set_model_params(p, np.ones((4, 16)))
    T.clear_model_params(p)
    assert p.calls == ["set_model_params_batch", "set_model_params_batch", "clear_model_params_batch"]
    # the CPU oracle plans every trajectory on the problem's model: the three verbs are not there
    from trajectoryoptimization_jl_amd import configs
    po = configs.cartpole_problem(batch=3, N=11, tf=0.5, lib=oracle)
    for call in (lambda: T.set_model_params(po, [T.Cartpole()] * 3), lambda: T.model_params(po), lambda: T.clear_model_params(po)):
        with pytest.raises(T.UnsupportedError, match="CPU oracle"):
            call()
