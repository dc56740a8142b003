"""Host side of to_policy_rollout, no GPU needed: the entry point is declared with the same version in the header, the ctypes mirror and
the Julia shim, it is bound for the HIP library only (the CPU oracle has no closed-loop rollout), the two structs mirror the header field
by field, and the Python wrapper checks shapes before it calls into a library."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
from trajectoryoptimization_jl_amd import configs

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "trajopt_hip.h").read_text()
SHIM = (ROOT / "julia" / "TrajOptHIP.jl").read_text()


def test_abi_7_everywhere():
    assert re.search(r"#define TO_ABI_VERSION 7\b", HEADER)
    assert T.capi.TO_ABI_VERSION == 7
    assert re.search(r"const TO_ABI_VERSION = Int32\(7\)", SHIM)
    assert re.search(r"^int to_policy_rollout\(", HEADER, flags=re.M)
    assert "ccall((:to_policy_rollout, lib), Cint," in SHIM


def test_bound_for_the_hip_library_only(oracle):
    assert "policy_rollout" in T.capi.HIP_ONLY and "policy_rollout" not in T.capi.SIGNATURES
    assert not hasattr(oracle.dll, "oracle_policy_rollout")
    p = configs.cartpole_problem(batch=2, N=11, tf=1.0, lib=oracle)
    with pytest.raises(NotImplementedError, match="HIP library"):
        T.policy_rollout(p, np.zeros((2, 1, 4)))


def _c_fields(name):
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + name + r"\s*;", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            out.append(decl.replace("const ", "").split(" ", 1)[1].replace("*", "").strip())
    return out


@pytest.mark.parametrize("cname, ctype, jname", [("to_policy_opts", "PolicyOpts", "PolicyOpts"), ("to_policy_result", "PolicyResult", "PolicyResult")])
def test_structs_mirror_the_header(cname, ctype, jname, tmp_path):
    fields = _c_fields(cname)
    assert [f for f, _ in getattr(T.capi, ctype)._fields_] == fields
    jbody = re.search(r"struct " + jname + r"\b.*?\n(.*?)\nend", SHIM, flags=re.S).group(1)
    assert [m.group(1) for m in re.finditer(r"^\s*(\w+)::", jbody, flags=re.M)] == fields
    # ... and has the size and the offsets the C compiler gives it
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trajopt_hip.h"\nint main(void) { printf("%zu", sizeof(' + cname + '));'
                   + "".join(f' printf(" %zu", offsetof({cname}, {f}));' for f in fields) + " return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run(["cc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    cls = getattr(T.capi, ctype)
    assert nums[0] == C.sizeof(cls)
    assert nums[1:] == [getattr(cls, f).offset for f in fields]


class _NoLibrary:
    """Stands where a library would: any call into it fails the test."""
    _fn = {"policy_rollout": None}

    def call(self, name, *args):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _problem_without_a_library(oracle):
    p = configs.cartpole_problem(batch=3, N=11, tf=1.0, lib=oracle)
    q = object.__new__(T.Problem)
    q.__dict__.update({k: v for k, v in p.__dict__.items() if k not in ("_h", "_lib")})
    q._lib, q._h = _NoLibrary(), C.c_void_p()
    return q


@pytest.mark.parametrize("shape", [(3, 4), (2, 5, 4), (3, 5, 3), (3, 0, 4), (3, 5, 4, 1)])
def test_wrongly_shaped_start_states_raise_before_the_library_is_called(shape, oracle):
    q = _problem_without_a_library(oracle)
    with pytest.raises(T.DimensionMismatch, match=r"X0s must be \[B=3, S >= 1, n=4\]"):
        T.policy_rollout(q, np.zeros(shape))


def test_clamp_and_plant_arguments_are_checked_on_the_host(oracle):
    q = _problem_without_a_library(oracle)
    ok = np.zeros((3, 2, 4))
    with pytest.raises(T.DimensionMismatch, match="u_min"):
        T.policy_rollout(q, ok, u_min=[-1.0, -1.0])
    with pytest.raises(T.ArgumentError, match="plant must be a Cartpole"):
        T.policy_rollout(q, ok, plant=T.DoubleIntegrator(1.0, 2))
    with pytest.raises(AssertionError, match="the library was called"):   # well-formed arguments do reach the library
        T.policy_rollout(q, ok, u_min=-1.0, u_max=[1.0], plant=T.Cartpole(mp=0.3))
