"""One tracking reference per trajectory (to_set_tracking_reference_batch, to_set_tracking_window, ...), everything that needs no GPU.

csrc/k_track.h is plain C++: tests/host_shim/track_lower_harness.cpp runs it thread by thread as a stand-alone program under
AddressSanitizer + UBSan, on arrays of exactly the sizes the entry points allocate, and compares every element of gl, as a 64-bit pattern,
with the plain loop of the host recipe; the same program puts every refusal of the two entry points to the host-only validation of
csrc/desc_lower.h (nothing is loaded into python).  Then the layers above: the five symbols in the header, the ctypes mirror, the Julia
shim and the built library, TO_ABI_MINOR still 1, and the Python wrappers' refusals, the 3-D dispatch of update_trajectory and mpc_run's
bookkeeping of the window starts against a library that only records its calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajectoryoptimization_jl_amd import api

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
HEADER = (ROOT / "include" / "trajopt_hip.h").read_text()
SHIM = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
SYMBOLS = {
    "set_tracking_reference_batch": ["to_handle* h", "int32_t Nref", "const double* Xref", "const double* Uref", "const int32_t* start", "int32_t end_mode"],
    "set_tracking_window": ["to_handle* h", "const int32_t* start"],
    "get_tracking_window": ["to_handle* h", "int32_t* Nref", "int32_t* end_mode", "int32_t* start"],
    "clear_tracking_reference_batch": ["to_handle* h"],
    "get_cost_linear_batch": ["to_handle* h", "int32_t cost_id", "double* q", "double* r"],
}


# ------------------------------------------------------------------------------------------------ the kernel and the validation, on the host
def test_kernel_under_sanitizers_equals_the_host_recipe_and_every_refusal_has_its_class(tmp_path):
    """(n, m, N) in {(2,1,4), (4,1,21), (13,4,15)} diagonal kinds + (4,2,9) dense QUADRATIC x B in {1, 64, 65, 130} x Nref in {N, N+7} x three
    kinds of starts x Uref given / NULL x one / many row groups; r rows, unused costs and lanes behind B untouched; the refusals."""
    exe = tmp_path / "track_lower_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "tests" / "host_shim"), "-I", str(CSRC), str(ROOT / "tests" / "host_shim" / "track_lower_harness.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert int(words[words.index("fails") + 1]) == 0
    assert int(words[words.index("checks") + 1]) > 4 * 10 ** 6     # 4 shapes x 4 batches x 2 x 3 x 2 x 2, every element of every gl


def test_k_track_is_included_by_the_host_translation_unit_only():
    users = sorted(f.name for f in CSRC.glob("*") if f.suffix in (".hip", ".h") and '#include "k_track.h"' in f.read_text())
    assert users == ["trajopt_hip.hip"]
    text = (CSRC / "k_track.h").read_text()
    assert "#pragma clang fp contract(off)" in text and "__shared__" not in text and "atomic" not in text.replace("no atomics", "")


# ------------------------------------------------------------------------------------------------ header, mirror, shim, library
def test_symbols_in_header_mirror_shim_and_library():
    plain = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    capi = T.capi
    want = {"set_tracking_reference_batch": [capi._H, C.c_int32, capi._PD, capi._PD, capi._PI, C.c_int32], "set_tracking_window": [capi._H, capi._PI],
            "get_tracking_window": [capi._H, capi._PI, capi._PI, capi._PI], "clear_tracking_reference_batch": [capi._H],
            "get_cost_linear_batch": [capi._H, C.c_int32, capi._PD, capi._PD]}
    lib = T.load_hip_library()
    dll = C.CDLL(lib.path)
    for name, args in SYMBOLS.items():
        m = re.search(r"^int\s+to_" + name + r"\s*\(([^;]*?)\)\s*;", plain, flags=re.M | re.S)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == args, name
        assert capi.HIP_ONLY[name] == want[name], name
        assert name in capi.OPTIONAL_HIP and name not in capi.SIGNATURES, name            # found by symbol lookup; the oracle does not have them
        assert f"ccall((:to_{name}, lib), Cint," in SHIM, name
        assert hasattr(dll, "to_" + name) and name in lib._fn, name
        assert name in api.__all__ and callable(getattr(T, name)), name
    assert re.search(r"^#define TO_TRACK_END_REFUSE 0\b", HEADER, flags=re.M) and re.search(r"^#define TO_TRACK_END_HOLD\s+1\b", HEADER, flags=re.M)
    assert (capi.TRACK_END_REFUSE, capi.TRACK_END_HOLD) == (0, 1)
    assert re.search(r"^const TO_TRACK_END_REFUSE = Int32\(0\)", SHIM, flags=re.M) and re.search(r"^const TO_TRACK_END_HOLD = Int32\(1\)", SHIM, flags=re.M)
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_set_tracking_reference_batch; throw_error = false)" in SHIM
    assert "function TO.update_trajectory!(p::BatchProblem, Xref::Array{Float64,3}, Uref" in SHIM and "function set_tracking_window!(p::BatchProblem" in SHIM
    for fn in ("TO.update_trajectory!(p::BatchProblem, Xref", "set_tracking_window!", "tracking_window", "clear_tracking_reference_batch!", "cost_linear_batch"):
        body = SHIM[SHIM.index("function " + fn):]
        body = body[: body.index("\nend")]
        assert body.index("has_tracking_reference_batch() ||") < body.index("ccall"), fn
    for verb in ("set_tracking_window!", "tracking_window", "clear_tracking_reference_batch!", "cost_linear_batch", "has_tracking_reference_batch"):
        assert re.search(r"^export .*\b" + re.escape(verb), SHIM, flags=re.M | re.S), verb


def test_abi_numbers_did_not_move():
    assert re.search(r"^#define TO_ABI_VERSION 7$", HEADER, flags=re.M) and re.search(r"^#define TO_ABI_MINOR 1$", HEADER, flags=re.M)
    assert T.capi.TO_ABI_VERSION == 7 and T.capi.TO_ABI_MINOR == 1
    lib = T.load_hip_library()
    assert lib.abi_version() == 7 and lib.abi_minor() == 1
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    tail = history[history.index("to_set_tracking_reference_batch"):]
    for sym in SYMBOLS:
        assert "to_" + sym in tail, sym
    assert "TO_ABI_VERSION and TO_ABI_MINOR unchanged" in tail and "no existing struct changed" in tail and "symbol lookup" in tail


# ------------------------------------------------------------------------------------------------ the wrappers, against a recording library
class _Fake:
    """A problem whose library exports the entry points and records every call (no GPU)."""
    _fn = dict.fromkeys(("mpc_advance", "policy_rollout", "policy_rollout_mc", *SYMBOLS))

    def __init__(self, B=3, N=5, model=None):
        self.model = model or T.Cartpole()
        self.n, self.m = self.model.dims()
        self._lib, self.B, self.N, self.calls = self, B, N, []
        self.errstate_dim = self.model.errstate_dim
        self.x0 = np.zeros((B, self.n))
        self.status = np.zeros(B, np.int32)
        self.hybrid = False

    @staticmethod
    def _pd(a):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == np.float64
        return a.ctypes.data_as(C.POINTER(C.c_double))

    @staticmethod
    def _pi(a):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == np.int32
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    def _call(self, name, *args):
        B, n, m = self.B, self.n, self.m
        if name == "set_tracking_reference_batch":
            Nref, X, U, s, mode = args
            self.calls.append((name, dict(Nref=Nref, X=np.ctypeslib.as_array(X, (B, Nref, n)).copy(), U=None if U is None else np.ctypeslib.as_array(U, (B, Nref, m)).copy(),
                                          start=np.ctypeslib.as_array(s, (B,)).copy(), mode=mode)))
        elif name == "set_tracking_window":
            self.calls.append((name, np.ctypeslib.as_array(args[0], (B,)).copy()))
        elif name == "mpc_advance":
            out, s = args[4]._obj, args[1]._obj.shift
            self.calls.append((name,))
            np.ctypeslib.as_array(out.x_next, (B, n))[:] = 1.0
            np.ctypeslib.as_array(out.X_applied, (B, s + 1, n))[:] = 0.0
            np.ctypeslib.as_array(out.U_applied, (B, s, m))[:] = 0.0
            for f in ("J", "c_max", "dx_max"):
                np.ctypeslib.as_array(getattr(out, f), (B,))[:] = 0.0
            np.ctypeslib.as_array(out.status, (B,))[:] = self.status
            np.ctypeslib.as_array(out.k_limit, (B,))[:] = 0
        else:
            self.calls.append((name,))


class _Solver:
    def __init__(self, prob):
        self.prob, self.stats = prob, dict(iterations=np.zeros(prob.B, np.int32), status=np.zeros(prob.B, np.int32))

    def solve(self):
        self.prob.calls.append(("solve",))
        return self


X3 = np.arange(3 * 8 * 4, dtype=np.float64).reshape(3, 8, 4)


@pytest.mark.parametrize("args, kw, err, match", [
    ((np.zeros((3, 8)),), {}, T.DimensionMismatch, r"Xref must be \[B=3, Nref, n=4\]"),
    ((np.zeros((2, 8, 4)),), {}, T.DimensionMismatch, "Xref must be"),
    ((np.zeros((3, 8, 5)),), {}, T.DimensionMismatch, "Xref must be"),
    ((np.zeros((3, 0, 4)),), {}, T.DimensionMismatch, "Xref must be"),
    ((X3, np.zeros((3, 6, 1))), {}, T.DimensionMismatch, r"Uref must be \[B=3, Nref=8, m=1\] or \[B, Nref-1, m\]"),
    ((X3, np.zeros((3, 8, 2))), {}, T.DimensionMismatch, "Uref must be"),
    ((X3, np.zeros((8, 1))), {}, T.DimensionMismatch, "Uref must be"),
    ((X3,), dict(start=[1, 2]), T.DimensionMismatch, r"start must be an integer or \[B=3\]"),
    ((X3,), dict(start=np.ones((3, 1), int)), T.DimensionMismatch, "start must be"),
    ((X3,), dict(start=1.5), T.ArgumentError, "start must be an integer"),
    ((X3,), dict(start=True), T.ArgumentError, "start must be an integer"),
    ((X3,), dict(end="clamp"), T.ArgumentError, "end must be one of"),
    ((X3,), dict(end=1), T.ArgumentError, "end must be one of"),
])
def test_wrapper_refuses_bad_shapes_before_the_library_sees_them(args, kw, err, match):
    p = _Fake()
    with pytest.raises(err, match=match):
        T.set_tracking_reference_batch(p, *args, **kw)
    assert p.calls == []
    with pytest.raises((T.DimensionMismatch, T.ArgumentError)):
        T.set_tracking_window(p, [1, 2])
    with pytest.raises(T.ArgumentError):
        T.set_tracking_window(p, 2.0)
    assert p.calls == []


def test_wrapper_passes_well_formed_arguments_on():
    p = _Fake()
    U = -np.arange(3 * 7 * 1, dtype=np.float64).reshape(3, 7, 1)
    T.set_tracking_reference_batch(p, X3, U, start=[1, 2, 3], end="hold")
    (name, a), = p.calls
    assert name == "set_tracking_reference_batch" and (a["Nref"], a["mode"]) == (8, T.capi.TRACK_END_HOLD)
    np.testing.assert_array_equal(a["X"], X3)
    np.testing.assert_array_equal(a["U"][:, :7], U)                       # a short U is padded with a zero knot, as update_trajectory treats it
    np.testing.assert_array_equal(a["U"][:, 7], 0.0)
    np.testing.assert_array_equal(a["start"], [1, 2, 3])
    T.set_tracking_reference_batch(p, X3)                                 # no controls: NULL; start 1 for all; refuse
    a = p.calls[-1][1]
    assert a["U"] is None and a["mode"] == T.capi.TRACK_END_REFUSE
    np.testing.assert_array_equal(a["start"], [1, 1, 1])
    T.set_tracking_window(p, 4)
    np.testing.assert_array_equal(p.calls[-1][1], [4, 4, 4])
    T.set_tracking_window(p, np.array([2, 1, 3], dtype=np.int64))
    np.testing.assert_array_equal(p.calls[-1][1], [2, 1, 3])
    T.clear_tracking_reference_batch(p)
    assert p.calls[-1] == ("clear_tracking_reference_batch",) and p._tracking is None


def test_update_trajectory_dispatches_on_three_dimensions():
    p = _Fake()
    T.update_trajectory(p, X3, None, [2, 1, 1])
    (name, a), = p.calls
    assert name == "set_tracking_reference_batch" and a["U"] is None and a["mode"] == T.capi.TRACK_END_REFUSE
    np.testing.assert_array_equal(a["start"], [2, 1, 1])
    T.update_trajectory(p, X3, np.ones((3, 8, 1)))
    assert p.calls[-1][0] == "set_tracking_reference_batch" and p.calls[-1][1]["U"].shape == (3, 8, 1)
    np.testing.assert_array_equal(p.calls[-1][1]["start"], [1, 1, 1])


def test_an_older_library_refuses_by_symbol_name():
    old = _Fake()
    old._fn = dict.fromkeys(("mpc_advance", "policy_rollout"))
    for call, sym in ((lambda: T.set_tracking_reference_batch(old, X3), "to_set_tracking_reference_batch"), (lambda: T.set_tracking_window(old, 1), "to_set_tracking_window"),
                      (lambda: T.get_tracking_window(old), "to_get_tracking_window"), (lambda: T.clear_tracking_reference_batch(old), "to_clear_tracking_reference_batch"),
                      (lambda: T.get_cost_linear_batch(old, 0), "to_get_cost_linear_batch")):
        with pytest.raises(T.UnsupportedError, match="exports " + sym):
            call()
    assert old.calls == []


def _windows(p):
    return [c[1] for c in p.calls if c[0] == "set_tracking_window"]


def test_mpc_run_moves_the_windows_of_the_trajectories_that_moved():
    p = _Fake(B=3, N=5)
    T.set_tracking_reference_batch(p, X3, start=[1, 2, 3], end="hold")       # Nref = 8
    p.calls.clear()
    p.status[:] = [0, T.capi.STATE_LIMIT, 0]                                # trajectory 1 leaves the limits in every period: it never moves
    T.mpc_run(_Solver(p), 3, shift=2)
    assert [c[0] for c in p.calls] == ["solve", "mpc_advance", "set_tracking_window"] * 3
    w = _windows(p)
    np.testing.assert_array_equal(w, [[3, 2, 5], [5, 2, 7], [7, 2, 8]])     # hold: a start behind the reference stays on its last knot (Nref = 8)
    np.testing.assert_array_equal(p._tracking["start"], [7, 2, 8])
    # refuse: the window that would run off the end raises BEFORE the call (start - 1 + N <= Nref: the last start that fits is 4)
    q = _Fake(B=3, N=5)
    T.set_tracking_reference_batch(q, X3, start=[1, 2, 1], end="refuse")
    q.calls.clear()
    with pytest.raises(T.ArgumentError, match=r"after period 1 the tracking window of trajectory 0 \(start 5, N = 5\) runs off the end"):
        T.mpc_run(_Solver(q), 3, shift=2)
    assert [c[0] for c in q.calls] == ["solve", "mpc_advance", "set_tracking_window", "solve", "mpc_advance"]
    np.testing.assert_array_equal(_windows(q), [[3, 4, 3]])
    # advance_reference=False: the caller moves the windows (or not)
    r = _Fake(B=3, N=5)
    T.set_tracking_reference_batch(r, X3, end="hold")
    r.calls.clear()
    T.mpc_run(_Solver(r), 2, advance_reference=False)
    assert [c[0] for c in r.calls] == ["solve", "mpc_advance"] * 2


def test_mpc_run_without_a_reference_makes_the_calls_it_always_made():
    p = _Fake(B=3, N=5)
    T.mpc_run(_Solver(p), 3, shift=1)
    assert [c[0] for c in p.calls] == ["solve", "mpc_advance"] * 3
    q = _Fake(B=3, N=5)                                                     # ... and after the reference was cleared
    T.set_tracking_reference_batch(q, X3)
    T.clear_tracking_reference_batch(q)
    q.calls.clear()
    T.mpc_run(_Solver(q), 2)
    assert [c[0] for c in q.calls] == ["solve", "mpc_advance"] * 2
