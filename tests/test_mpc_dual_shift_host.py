"""The kernel of to_mpc_shift_duals (csrc/k_mpc.h k_mpc_shift_duals) and its refusals (csrc/desc_lower.h validate_mpc_shift_duals), without
a GPU: tests/host_shim/mpc_dual_shift_harness.cpp compiles the same text for the host as a stand-alone program — once plain, once under
AddressSanitizer + UBSan — runs the kernel thread by thread on arrays of exactly the handle's sizes and compares every element, bit for
bit, with a scalar restatement (nothing is loaded into python).  Then the layers above: the symbol in the header, the ctypes mirror and
the Julia shim, and the Python wrapper's argument checks against a library that only records its calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import api
from trajectoryoptimization_jl_amd import configs

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
HEADER = (ROOT / "include" / "trajopt_hip.h").read_text()
SHIM = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
cap = T.capi
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "asan_ubsan"])
def test_kernel_and_refusals_equal_the_scalar_restatement(tmp_path, flags):
    """B in {1, 64, 70, 130} x three constraint tables (p = 1, 4, 6; nk = 1 .. 10) x s in {1, 2, 4, nk-1, nk, nk+3} x both tails x actions
    {NULL, all LEAVE, all SHIFT, all RESET, mixed}; padding lanes, left trajectories and unreset penalties keep their pattern; the refusals."""
    exe = tmp_path / "mpc_dual_shift_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *flags, "-I", str(ROOT / "tests" / "host_shim"), "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_shim" / "mpc_dual_shift_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert int(words[words.index("fails") + 1]) == 0
    assert int(words[words.index("checks") + 1]) > 3 * 10 ** 6


def test_kernel_is_plain_cxx_in_k_mpc():
    """In k_mpc.h, next to the shift it mirrors; no LDS, no atomics, no wave intrinsics — which is why the host shim can compile it."""
    text = (CSRC / "k_mpc.h").read_text()
    body = text[text.index("void __launch_bounds__(64) k_mpc_shift_duals"):]
    body = body[:body.index("\n}\n")]
    for word in ("__shared__", "atomic", "__ballot", "__shfl", "__syncthreads"):
        assert word not in body, word
    assert "if (b >= a.B) return;" in body


# ------------------------------------------------------------------------------------------------ header, mirror, shim
def test_symbol_in_header_mirror_shim_and_library():
    h = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"^int\s+to_mpc_shift_duals\s*\(([^;]*?)\)\s*;", h, flags=re.M | re.S)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["to_handle* h", "int32_t shift", "int32_t tail", "const int32_t* action"]
    assert "enum { TO_MPC_DUAL_TAIL_HOLD = 0, TO_MPC_DUAL_TAIL_ZERO = 1 };" in HEADER
    assert "enum { TO_MPC_DUAL_LEAVE = 0, TO_MPC_DUAL_SHIFT = 1, TO_MPC_DUAL_RESET = 2 };" in HEADER
    assert (cap.MPC_DUAL_TAIL_HOLD, cap.MPC_DUAL_TAIL_ZERO) == (0, 1) and (cap.MPC_DUAL_LEAVE, cap.MPC_DUAL_SHIFT, cap.MPC_DUAL_RESET) == (0, 1, 2)
    assert cap.HIP_ONLY["mpc_shift_duals"] == [cap._H, C.c_int32, C.c_int32, cap._PI]
    assert "mpc_shift_duals" in cap.OPTIONAL_HIP and "mpc_shift_duals" not in cap.SIGNATURES     # found by symbol lookup; the oracle does not have it
    lib = T.load_hip_library()
    assert hasattr(C.CDLL(lib.path), "to_mpc_shift_duals") and "mpc_shift_duals" in lib._fn
    assert "mpc_shift_duals" in api.__all__ and callable(T.mpc_shift_duals)
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_mpc_shift_duals; throw_error = false)" in SHIM
    assert "ccall((:to_mpc_shift_duals, lib), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32})," in SHIM
    for verb in ("mpc_shift_duals!", "has_mpc_shift_duals"):
        assert re.search(r"^export .*\b" + re.escape(verb), SHIM, flags=re.M | re.S), verb
    for name, val in (("TO_MPC_DUAL_TAIL_HOLD", 0), ("TO_MPC_DUAL_TAIL_ZERO", 1), ("TO_MPC_DUAL_LEAVE", 0), ("TO_MPC_DUAL_SHIFT", 1), ("TO_MPC_DUAL_RESET", 2)):
        assert re.search(rf"^const {name} = Int32\({val}\)", SHIM, flags=re.M), name


def test_abi_numbers_did_not_move_and_the_history_says_so():
    assert re.search(r"^#define TO_ABI_VERSION 7$", HEADER, flags=re.M) and re.search(r"^#define TO_ABI_MINOR 1$", HEADER, flags=re.M)
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    tail = history[history.index("to_mpc_shift_duals"):]
    assert "symbol lookup" in tail and "no existing struct" in tail
    about_options = HEADER[HEADER.index("Options are validated"):HEADER.index("int to_set_options")]
    assert "to_mpc_shift_duals" in about_options                     # who rewrites the penalties: the new case is named
    assert "are not shifted" in T.mpc_advance.__doc__ and "mpc_shift_duals" in T.mpc_advance.__doc__


# ------------------------------------------------------------------------------------------------ the wrapper, against a recording library
class _Fake:
    """A problem whose library exports the entry point and records every call (no GPU)."""
    _fn = dict.fromkeys(("mpc_advance", "policy_rollout", "mpc_shift_duals"))

    def __init__(self, B=4, N=11):
        self._lib, self.B, self.N, self.calls = self, B, N, []

    @staticmethod
    def _pi(a):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == np.int32
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    def _call(self, name, *args):
        s, tail, act = args
        self.calls.append((name, s, tail, None if act is None else np.ctypeslib.as_array(act, (self.B,)).copy()))


@pytest.mark.parametrize("kw, err, match", [
    (dict(shift=0), T.ArgumentError, r"shift must be an integer in 1 \.\. N-2 = 9"),
    (dict(shift=10), T.ArgumentError, "shift must be"),
    (dict(shift=2.0), T.ArgumentError, "shift must be"),
    (dict(shift=True), T.ArgumentError, "shift must be"),
    (dict(shift=1, tail="fill"), T.ArgumentError, r"tail must be one of \['hold', 'zero'\]"),
    (dict(shift=1, tail=0), T.ArgumentError, "tail must be one of"),
    (dict(shift=1, action=[1, 1, 1]), T.DimensionMismatch, r"action must be \[B=4\]"),
    (dict(shift=1, action=1), T.DimensionMismatch, "action must be"),
    (dict(shift=1, action=[0, 1, 2, 3]), T.ArgumentError, "action must hold 0 / 1 / 2 or .*got 3"),
    (dict(shift=1, action=[0, 1, 2, -1]), T.ArgumentError, "got -1"),
    (dict(shift=1, action=[0.0, 1.0, 2.0, 1.0]), T.ArgumentError, "action must hold"),
    (dict(shift=1, action=[True, False, True, True]), T.ArgumentError, "action must hold"),
    (dict(shift=1, action=["shift", "leave", "reset", "hold"]), T.ArgumentError, "got 'hold'"),
])
def test_wrapper_refuses_bad_input_before_the_library_sees_it(kw, err, match):
    p = _Fake()
    with pytest.raises(err, match=match):
        T.mpc_shift_duals(p, **kw)
    assert p.calls == []


def test_wrapper_passes_well_formed_arguments_on():
    p = _Fake()
    T.mpc_shift_duals(p, 3)
    assert p.calls[-1][:3] == ("mpc_shift_duals", 3, cap.MPC_DUAL_TAIL_HOLD) and p.calls[-1][3] is None      # NULL: shift for all, no upload
    T.mpc_shift_duals(p, np.int64(9), tail="zero", action=np.array([2, 0, 1, 1], np.int64))
    assert p.calls[-1][:3] == ("mpc_shift_duals", 9, cap.MPC_DUAL_TAIL_ZERO)
    np.testing.assert_array_equal(p.calls[-1][3], [2, 0, 1, 1])
    assert p.calls[-1][3].dtype == np.int32
    T.mpc_shift_duals(p, 1, action=["leave", "shift", "reset", "shift"])
    np.testing.assert_array_equal(p.calls[-1][3], [0, 1, 2, 1])


def test_an_oracle_backed_problem_and_an_older_library_refuse(oracle):
    po = configs.cartpole_problem(batch=2, N=11, tf=1.0, constrained=True, lib=oracle)
    with pytest.raises(NotImplementedError, match="HIP library"):
        T.mpc_shift_duals(po, 1)
    old = _Fake()
    old._fn = dict.fromkeys(("mpc_advance", "policy_rollout"))
    with pytest.raises(T.UnsupportedError, match="exports to_mpc_shift_duals"):
        T.mpc_shift_duals(old, 1)
    assert old.calls == []
