"""The receding-horizon step (to_mpc_advance, T.mpc_advance, T.mpc_run), everything that needs no GPU.

csrc/k_mpc.h — the write-back, both guesses of the shift and the x0 copy — is plain C++: tests/host_shim/mpc_shift_harness.cpp runs it
thread by thread as a stand-alone program under AddressSanitizer + UBSan, on arrays of exactly the sizes the entry point allocates, and
compares every result bit for bit with the plain loop  Unew[k] = k + s <= N-2 ? V[k + s] : tail  (nothing is loaded into python).  Then
the layers above: the symbol and the two structs in the header, the ctypes mirror and the Julia shim, their sizes from a compiled C snippet,
TO_ABI_MINOR still 1, and the Python wrappers' refusals and the bookkeeping of mpc_run against a library that only records its calls."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajectoryoptimization_jl_amd import api, configs

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
HEADER = (ROOT / "include" / "trajopt_hip.h").read_text()
SHIM = (ROOT / "julia" / "TrajOptHIP.jl").read_text()
OPTS_FIELDS = ["shift", "guess", "tail", "reserved", "u_fill"]
RESULT_FIELDS = ["x_next", "X_applied", "U_applied", "J", "c_max", "dx_max", "status", "k_limit"]


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernels_under_sanitizers_equal_the_plain_loop(tmp_path):
    """(n, m, N) in {(2,1,4), (4,1,21), (13,4,15)} x B in {1, 64, 65, 130} x s in {1, 2, N-2} x both guesses x both tails x chunks of one
    wave and of all waves; lanes behind B and trajectories with a nonzero status unchanged; the host-layout gathers; k_mpc_x0_in."""
    exe = tmp_path / "mpc_shift_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "tests" / "host_shim"), "-I", str(CSRC), str(ROOT / "tests" / "host_shim" / "mpc_shift_harness.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    words = r.stdout.split()
    assert int(words[words.index("fails") + 1]) == 0
    assert int(words[words.index("checks") + 1]) > 10 ** 6     # 3 shapes x 4 batches x 3 (2) shifts x 2 x 2 x 2, every element of every array


def test_k_mpc_is_included_by_the_host_translation_unit_only():
    """The kernels are non-template __global__ functions: a second translation unit that included the header would define them twice."""
    users = sorted(f.name for f in CSRC.glob("*") if f.suffix in (".hip", ".h") and '#include "k_mpc.h"' in f.read_text())
    assert users == ["trajopt_hip.hip"]


# ------------------------------------------------------------------------------------------------ header, mirror, shim
def _c_fields(name):
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + name + r"\s*;", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            out.append(decl.replace("const ", "").split(" ", 1)[1].replace("*", "").strip())
    return out


def _julia_fields(name):
    body = re.search(r"struct " + name + r"\b.*?\n(.*?)\nend", SHIM, flags=re.S).group(1)
    return [m.group(1) for m in re.finditer(r"^\s*(\w+)::", body, flags=re.M)], re.findall(r"::(\w+(?:\{\w+\})?)", body)


def test_structs_mirror_the_header(tmp_path):
    assert _c_fields("to_mpc_opts") == OPTS_FIELDS and _c_fields("to_mpc_result") == RESULT_FIELDS
    assert [f for f, _ in T.capi.MpcOpts._fields_] == OPTS_FIELDS and [f for f, _ in T.capi.MpcResult._fields_] == RESULT_FIELDS
    names, types = _julia_fields("MpcOpts")
    assert names == OPTS_FIELDS and types == ["Int32"] * 4 + ["Ptr{Float64}"]
    names, types = _julia_fields("MpcResult")
    assert names == RESULT_FIELDS and types == ["Ptr{Float64}"] * 6 + ["Ptr{Int32}"] * 2
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trajopt_hip.h"\nint main(void) { printf("%zu %zu", sizeof(to_mpc_opts), sizeof(to_mpc_result));'
                   + "".join(f' printf(" %zu", offsetof(to_mpc_opts, {f}));' for f in OPTS_FIELDS)
                   + "".join(f' printf(" %zu", offsetof(to_mpc_result, {f}));' for f in RESULT_FIELDS)
                   + ' printf(" %d %d %d %d", TO_MPC_GUESS_CLOSED_LOOP, TO_MPC_GUESS_NOMINAL, TO_MPC_TAIL_HOLD, TO_MPC_TAIL_FILL); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["cc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(T.capi.MpcOpts) == 24 and nums[1] == C.sizeof(T.capi.MpcResult) == 64
    assert nums[2:7] == [getattr(T.capi.MpcOpts, f).offset for f in OPTS_FIELDS] == [0, 4, 8, 12, 16]
    assert nums[7:15] == [getattr(T.capi.MpcResult, f).offset for f in RESULT_FIELDS] == [8 * i for i in range(8)]
    assert nums[15:] == [T.capi.MPC_GUESS_CLOSED_LOOP, T.capi.MPC_GUESS_NOMINAL, T.capi.MPC_TAIL_HOLD, T.capi.MPC_TAIL_FILL] == [0, 1, 0, 1]
    for name, val in (("TO_MPC_GUESS_CLOSED_LOOP", 0), ("TO_MPC_GUESS_NOMINAL", 1), ("TO_MPC_TAIL_HOLD", 0), ("TO_MPC_TAIL_FILL", 1)):
        assert re.search(rf"^const {name} = Int32\({val}\)", SHIM, flags=re.M), name


def test_symbol_in_header_mirror_shim_and_library():
    m = re.search(r"^int\s+to_mpc_advance\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.M | re.S)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "to_handle* h", "const double* x_meas", "const to_mpc_opts* mpc", "const to_policy_opts* popts", "const to_policy_noise* noise", "const to_mpc_result* out"]
    capi = T.capi
    assert capi.HIP_ONLY["mpc_advance"] == [capi._H, capi._PD, C.POINTER(capi.MpcOpts), C.POINTER(capi.PolicyOpts), C.POINTER(capi.PolicyNoise),
                                            C.POINTER(capi.MpcResult)]
    assert "mpc_advance" in capi.OPTIONAL_HIP and "mpc_advance" not in capi.SIGNATURES     # found by symbol lookup; the oracle does not have it
    assert "Libdl.dlsym(Libdl.dlopen(lib), :to_mpc_advance; throw_error = false)" in SHIM
    assert ("ccall((:to_mpc_advance, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{MpcOpts}, Ref{PolicyOpts}, Ref{PolicyNoise}, Ref{MpcResult}),"
            in SHIM)
    body = SHIM[SHIM.index("function mpc_advance!"):]
    body = body[: body.index("\nend")]
    assert body.index("has_mpc_advance() ||") < body.index("ccall") and body.index("DimensionMismatch") < body.index("ccall")
    for verb in ("mpc_advance!", "has_mpc_advance", "MpcOpts", "MpcResult"):
        assert re.search(r"^export .*\b" + re.escape(verb), SHIM, flags=re.M | re.S), verb
    lib = T.load_hip_library()
    assert hasattr(C.CDLL(lib.path), "to_mpc_advance") and "mpc_advance" in lib._fn
    for n in ("mpc_advance", "MpcAdvance", "mpc_run", "MpcRun"):
        assert n in api.__all__ and callable(getattr(T, n))


def test_abi_minor_did_not_move():
    assert re.search(r"^#define TO_ABI_VERSION 7$", HEADER, flags=re.M) and re.search(r"^#define TO_ABI_MINOR 1$", HEADER, flags=re.M)
    assert T.capi.TO_ABI_VERSION == 7 and T.capi.TO_ABI_MINOR == 1
    assert re.search(r"^const TO_ABI_VERSION = Int32\(7\)", SHIM, flags=re.M) and re.search(r"^const TO_ABI_MINOR = Int32\(1\)", SHIM, flags=re.M)
    lib = T.load_hip_library()
    assert lib.abi_version() == 7 and lib.abi_minor() == 1
    history = HEADER[HEADER.index("ABI history"):HEADER.index("#define TO_ABI_VERSION")]
    assert "to_mpc_advance" in history and "to_mpc_opts" in history and "to_mpc_result" in history
    assert "no existing struct changed in size" in history and "symbol lookup" in history[history.index("to_mpc_advance"):]


# ------------------------------------------------------------------------------------------------ the wrappers, against a recording library
class _Fake:
    """A problem whose library exports the entry point, records every call and answers an advance with recognisable arrays (no GPU)."""
    _fn = dict.fromkeys(("mpc_advance", "policy_rollout", "policy_rollout_mc"))

    def __init__(self, B=3, N=11, model=None):
        self.model = model or T.Cartpole()
        self.n, self.m = self.model.dims()
        self._lib, self.B, self.N, self.calls = self, B, N, []
        self.errstate_dim = self.model.errstate_dim
        self.x0 = np.zeros((B, self.n))
        self.status = np.zeros(B, np.int32)

    @staticmethod
    def _pd(a):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == np.float64
        return a.ctypes.data_as(C.POINTER(C.c_double))

    @staticmethod
    def _pi(a):
        assert a.flags["C_CONTIGUOUS"] and a.dtype == np.int32
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    def _call(self, name, *args):
        if name != "mpc_advance":
            self.calls.append((name,))
            return
        xm, mo, po, nz, out = args
        mo, po, out = mo._obj, po._obj, out._obj
        s, t = mo.shift, len([c for c in self.calls if c[0] == "mpc_advance"])
        self.calls.append(("mpc_advance", dict(
            x_meas=None if xm is None else np.ctypeslib.as_array(xm, (self.B, self.n)).copy(), shift=s, guess=mo.guess, tail=mo.tail, reserved=mo.reserved,
            u_fill=None if not mo.u_fill else np.ctypeslib.as_array(mo.u_fill, (self.m,)).copy(), alpha=po.alpha, refresh_gains=po.refresh_gains,
            noise=None if nz is None else (nz._obj.seed, nz._obj.traj_offset, nz._obj.sample_offset, bool(nz._obj.sigma_w), bool(nz._obj.sigma_v)))))
        np.ctypeslib.as_array(out.x_next, (self.B, self.n))[:] = 100 * t + 99
        np.ctypeslib.as_array(out.X_applied, (self.B, s + 1, self.n))[:] = 100 * t + np.arange(s + 1)[None, :, None]
        np.ctypeslib.as_array(out.U_applied, (self.B, s, self.m))[:] = -(100 * t + np.arange(s)[None, :, None])
        for f in ("J", "c_max", "dx_max"):
            np.ctypeslib.as_array(getattr(out, f), (self.B,))[:] = t
        np.ctypeslib.as_array(out.status, (self.B,))[:] = self.status
        np.ctypeslib.as_array(out.k_limit, (self.B,))[:] = 0


def _advances(p):
    return [c[1] for c in p.calls if c[0] == "mpc_advance"]


@pytest.mark.parametrize("kw, err, match", [
    (dict(shift=0), T.ArgumentError, r"shift must be an integer in 1 \.\. N-2 = 9"),
    (dict(shift=10), T.ArgumentError, "shift must be"),
    (dict(shift=1.5), T.ArgumentError, "shift must be"),
    (dict(shift=True), T.ArgumentError, "shift must be"),
    (dict(guess="closed loop"), T.ArgumentError, "guess must be one of"),
    (dict(guess=0), T.ArgumentError, "guess must be one of"),
    (dict(tail="zero"), T.ArgumentError, "tail must be one of"),
    (dict(tail="fill"), T.ArgumentError, "needs u_fill"),
    (dict(tail="fill", u_fill=[0.0, 0.0]), T.DimensionMismatch, r"u_fill must be a scalar or \[m=1\]"),
    (dict(tail="fill", u_fill=np.zeros((1, 1))), T.DimensionMismatch, "u_fill must be"),
    (dict(tail="fill", u_fill=np.inf), T.ArgumentError, "u_fill must be finite"),
    (dict(x_meas=np.zeros((2, 4))), T.DimensionMismatch, r"x_meas must be \[B=3, n=4\] or \[n\]"),
    (dict(x_meas=np.zeros((3, 5))), T.DimensionMismatch, "x_meas must be"),
    (dict(x_meas=np.zeros((3, 1, 4))), T.DimensionMismatch, "x_meas must be"),
    (dict(u_min=[0.0, 0.0]), T.DimensionMismatch, None),
    (dict(noise=0.1), T.ArgumentError, "must be a PolicyNoise"),
    (dict(noise=T.PolicyNoise(1, sigma_w=[0.1] * 3)), T.DimensionMismatch, r"sigma_w must be a scalar or \[ne=4\]"),
    (dict(plant=T.DoubleIntegrator(1.0, 2)), T.ArgumentError, "plant must be a Cartpole"),
])
def test_wrapper_refuses_bad_input_before_the_library_sees_it(kw, err, match):
    p = _Fake()
    with pytest.raises(err, match=match):
        T.mpc_advance(p, **kw)
    assert p.calls == []


def test_wrapper_passes_well_formed_arguments_on():
    p = _Fake()
    p.status[:] = [0, T.capi.STATE_LIMIT, 0]
    xm = np.arange(12.0).reshape(3, 4)
    r = T.mpc_advance(p, xm, shift=3, guess="nominal", tail="fill", u_fill=0.25, alpha=0.5, refresh_gains=False,
                      noise=T.PolicyNoise(7, sigma_w=0.1, sample_offset=4))
    (a,) = _advances(p)
    np.testing.assert_array_equal(a["x_meas"], xm)
    assert (a["shift"], a["guess"], a["tail"], a["reserved"]) == (3, T.capi.MPC_GUESS_NOMINAL, T.capi.MPC_TAIL_FILL, 0)
    np.testing.assert_array_equal(a["u_fill"], [0.25])
    assert (a["alpha"], a["refresh_gains"], a["noise"]) == (0.5, 0, (7, 0, 4, True, False))
    assert r.x_next.shape == (3, 4) and r.X.shape == (3, 4, 4) and r.U.shape == (3, 3, 1)
    assert all(getattr(r, k).shape == (3,) for k in ("J", "c_max", "dx_max", "status", "k_limit")) and r.status.dtype == r.k_limit.dtype == np.int32
    # the host's copy of x0 follows the handle: the trajectory beyond the limit keeps its own
    np.testing.assert_array_equal(p.x0, [[99.0] * 4, [0.0] * 4, [99.0] * 4])
    q = _Fake()
    T.mpc_advance(q, np.arange(4.0))                               # one measured state for the whole batch
    (a,) = _advances(q)
    np.testing.assert_array_equal(a["x_meas"], np.tile(np.arange(4.0), (3, 1)))
    assert (a["shift"], a["guess"], a["tail"], a["u_fill"], a["noise"]) == (1, 0, 0, None, None) and (a["alpha"], a["refresh_gains"]) == (0.0, 1)
    T.mpc_advance(q)                                               # no measurement: NULL, the handle's own x0
    assert _advances(q)[1]["x_meas"] is None


def test_an_oracle_backed_problem_and_an_older_library_refuse(oracle):
    po = configs.cartpole_problem(batch=2, N=11, tf=1.0, lib=oracle)
    with pytest.raises(NotImplementedError, match="HIP library"):
        T.mpc_advance(po)
    with pytest.raises(NotImplementedError, match="HIP library"):
        T.mpc_run(T.iLQRSolver(po, iterations=1), 1)
    old = _Fake()
    old._fn = dict.fromkeys(("policy_rollout", "policy_rollout_mc"))
    with pytest.raises(T.UnsupportedError, match="exports to_mpc_advance"):
        T.mpc_advance(old)


class _Solver:
    def __init__(self, prob):
        self.prob, self.stats, self.n = prob, dict(iterations=np.zeros(prob.B, np.int32), status=np.zeros(prob.B, np.int32)), 0

    def solve(self):
        self.prob.calls.append(("solve",))
        self.n += 1
        self.stats["iterations"][:] = 10 * self.n + np.arange(self.prob.B)
        self.stats["status"][:] = T.capi.SOLVE_SUCCEEDED
        return self


@pytest.mark.parametrize("shift", [1, 2])
def test_mpc_run_bookkeeping(shift):
    p = _Fake(B=3, N=11)
    sol, hooks = _Solver(p), []
    steps = 4

    def before(prob, t):
        assert prob is p
        hooks.append(t)
        p.calls.append(("before", t))
    xt = np.arange(12.0).reshape(3, 4)
    rec = T.mpc_run(sol, steps, shift=shift, x_true=xt, noise=T.PolicyNoise(5, sigma_w=0.01), before_solve=before, alpha=0.25, tail="fill", u_fill=0.0)
    assert hooks == [0, 1, 2, 3]
    assert [c[0] for c in p.calls] == ["before", "solve", "mpc_advance"] * steps            # the hook once per period, before its solve
    adv = _advances(p)
    assert [a["noise"][2] for a in adv] == [0, 1, 2, 3] and all(a["noise"][:2] == (5, 0) for a in adv)   # sample_offset = the period
    np.testing.assert_array_equal(adv[0]["x_meas"], xt)
    assert all(a["x_meas"] is None for a in adv[1:])                                         # afterwards the true state is the handle's x0
    assert all((a["shift"], a["alpha"], a["tail"]) == (shift, 0.25, T.capi.MPC_TAIL_FILL) for a in adv)
    assert rec.X_cl.shape == (3, steps * shift + 1, 4) and rec.U_cl.shape == (3, steps * shift, 1)
    assert rec.iterations.shape == rec.status.shape == rec.advance_status.shape == rec.k_limit.shape == (steps, 3)
    assert rec.iterations.dtype == rec.status.dtype == np.int32
    np.testing.assert_array_equal(rec.iterations, 10 * np.arange(1, steps + 1)[:, None] + np.arange(3)[None, :])
    np.testing.assert_array_equal(rec.status, T.capi.SOLVE_SUCCEEDED)
    # period t contributes its knots 1 .. shift; knot 0 of the record is the first period's measured state
    want_x = np.concatenate([[0.0]] + [100.0 * t + np.arange(1, shift + 1) for t in range(steps)])
    want_u = np.concatenate([-(100.0 * t + np.arange(shift)) for t in range(steps)])
    np.testing.assert_array_equal(rec.X_cl[1, :, 2], want_x)
    np.testing.assert_array_equal(rec.U_cl[2, :, 0], want_u)
    # an offset of the caller's is kept: period t draws at sample_offset + t
    p2 = _Fake()
    T.mpc_run(_Solver(p2), 2, noise=T.PolicyNoise(5, sigma_v=0.01, traj_offset=64, sample_offset=10))
    assert [a["noise"] for a in _advances(p2)] == [(5, 64, 10, False, True), (5, 64, 11, False, True)]
    with pytest.raises(T.ArgumentError, match="steps must be >= 1"):
        T.mpc_run(_Solver(_Fake()), 0)
