"""The closed-loop policy rollout KERNEL (csrc/k_policy.h) and the kernels of to_mpc_advance (csrc/k_mpc.h) compiled for the host
(tests/host_shim/policy_harness.cpp) and run thread by thread in the launch sequences of to_policy_rollout and to_mpc_advance, with
every array at exactly the length the library's plan_policy / plan_mpc (csrc/path_plan.h) gives it.  No GPU needed.

* ``test_sanitized_program``: the harness as a stand-alone program under AddressSanitizer + UBSan walks the constrained Quadrotor (C5:
  GoalConstraint on C5_GOAL_INDS + second-order-cone NormConstraint) and a constrained Cartpole over N in {4, 21}, B in {1, 64, 65, 130,
  1024}, S in {1, 3, 33, 64, 70}, both lane maps, chunks of one wave and of all waves, with and without the trajectories, NZ in {0, 4, 7},
  and to_mpc_advance with s in {1, N-2}, both guesses, both tails.  An address outside an array is a sanitizer report; a store where none
  belongs, or two lane maps that disagree in one bit, is a failed check.
* ``test_constrained_quadrotor_matches_the_restatement``: the unsanitized build against tests/policy_ref.py on a Quadrotor C5 problem solved
  by the oracle's ALSolver, gains from the oracle's phase API: the same comparison, tolerance and conditions as
  tests/test_gpu_policy_rollout.py makes on the MI355X — knot_violation with an indexed GoalConstraint and a cone on a 13-state model against
  the oracle's max_violation.
* ``test_plan_policy`` / ``test_plan_mpc``: the lengths the entry points allocate, against their arithmetic written out here.
* ``test_solve_path_of_the_large_batch``: which kernel instances a constrained Quadrotor handle of 1024 trajectories selects (profiles/
  policy_constrained.md)."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

import policy_ref as R

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_shim" / "policy_harness.cpp"
INCLUDES = ["-I", str(ROOT / "tests" / "host_shim"), "-I", str(ROOT / "trajectoryoptimization.jl_amd" / "csrc")]
PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("policyhost") / "libpolicy_host.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", *INCLUDES, "-o", str(so), str(SRC)], check=True)
    lib = C.CDLL(str(so))
    lib.policy_host_rollout.restype = C.c_int
    lib.policy_host_rollout.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, PD, PD, PD, PD, PD, C.c_double, PD, PD, PD, PD, PD, PD, PD, PD, PI, PI]
    lib.policy_host_last_error.restype = C.c_char_p
    lib.policy_host_plan.restype = None
    lib.policy_host_solve_path.restype = None
    return lib


def test_sanitized_program(tmp_path):
    """Nothing with a sanitizer is loaded into Python: the program has its own main and runs as a child process."""
    exe = tmp_path / "policy_asan"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-w",
                    "-DPOLICY_HARNESS_MAIN", *INCLUDES, "-o", str(exe), str(SRC)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    tail = res.stdout[-3000:] + res.stderr[-6000:]
    assert res.returncode == 0, tail
    assert "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, tail
    m = re.search(r"checks (\d+) fails (\d+)\s*$", res.stdout)
    assert m, tail
    assert int(m.group(1)) > 100000 and int(m.group(2)) == 0, tail


# ------------------------------------------------------------------------------------------------ the plan
def plan(host, n, m, N, B, S, lane_map=0, chunk=0, pieces=0, s=1):
    out, mpc = (C.c_longlong * 12)(), (C.c_longlong * 5)()
    host.policy_host_plan(n, m, N, B, S, lane_map, chunk, pieces, s, out, mpc)
    keys = ["packed", "TPW", "WPT", "waves", "SB", "x0s_len", "sample_len", "chunk", "xw_len", "uw_len", "rollout_stage_len", "lds_bytes"]
    return dict(zip(keys, out)), dict(zip(["cx", "cX", "cU", "stage_len", "row_groups"], mpc))


@pytest.mark.parametrize("n,m,N,pieces", [(13, 4, 21, 26), (13, 4, 4, 26), (4, 1, 31, 0), (4, 2, 21, 0)])
def test_plan_policy(host, n, m, N, pieces):
    """Lane map, waves, chunk and every length, against the arithmetic of the entry points written out: the packed map holds 64 // S
    trajectories per wave, the uniform one ceil(S / 64) waves per trajectory; the staging pair is 32 MiB at most, or the override; the
    LDS is two buffers of whole 64-piece DMA instructions."""
    Lx, Lu = N * n, (N - 1) * m
    for B in (1, 64, 65, 130, 1024):
        for S in (1, 3, 32, 33, 64, 70):
            for lane_map in (0, 1, 2):
                for chunk in (0, 1, 5):
                    p, _ = plan(host, n, m, N, B, S, lane_map, chunk, pieces)
                    packed = (S <= 32 or (lane_map == 1 and S <= 64)) and lane_map != 2
                    TPW = 64 // S if packed else 0
                    waves = -(-B // TPW) if packed else B * -(-S // 64)
                    want_chunk = min(waves, chunk if chunk else max(1, (32 << 20) // (64 * (Lx + Lu) * 8)))
                    TW = TPW if packed else 1
                    lds = 2 * 8 * (-(-(TW * pieces) // 64) * 64 * 2) if pieces else 0
                    want = dict(packed=int(packed), TPW=TPW, WPT=-(-S // 64), waves=waves, SB=S * B, x0s_len=S * B * n, sample_len=S * B,
                                chunk=want_chunk, xw_len=want_chunk * Lx * 64, uw_len=want_chunk * Lu * 64,
                                rollout_stage_len=want_chunk * 64 * (Lx + Lu), lds_bytes=lds)
                    assert p == want, (B, S, lane_map, chunk)
                    assert waves * 64 >= S * B and lds <= 64 * 1024   # every sample has a lane; the LDS fits a workgroup's 64 KiB


def test_plan_mpc(host):
    for (n, m, N) in ((13, 4, 21), (4, 1, 4), (2, 1, 31)):
        for B in (1, 65, 1024):
            for s in (1, N - 2):
                _, q = plan(host, n, m, N, B, 1, s=s)
                assert q == dict(cx=n * B, cX=n * (s + 1) * B, cU=m * s * B, stage_len=n * B + n * (s + 1) * B + m * s * B,
                                 row_groups=min(32, max((N - 1) * m, (s + 1) * n)))


def test_solve_path_of_the_large_batch(host):
    """B = 1024 constrained Quadrotor trajectories on 256 compute units select the kernel instances B = 65 selects: the MFMA backward pass
    with compaction, 16 step sizes per base round, the deep forward-wave shape (20 step sizes x 3 trajectories) as two-wave workgroups from
    the first batch step, whole candidates stored.  (The first difference comes at 1537 active trajectories: one-wave workgroups.)"""
    def path(B, active):
        info, step = (C.c_int32 * 8)(), (C.c_int32 * 6)()
        host.policy_host_solve_path(B, 21, 256, active, info, step)
        return list(info), list(step)
    assert path(1024, 1024) == path(65, 65) == ([1, 0, 1, 16, 2, 0, 1, 1], [0, 20, 3, 1, 1, 0])
    assert path(1024, 256)[1] == path(65, 16)[1] == [0, 20, 3, 1, 1, 0]
    assert path(2048, 1536)[1] == [0, 20, 3, 1, 1, 0] and path(2048, 1537)[1] == [0, 20, 3, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ numbers
S_VALUES = [1, 3, 64, 70]
S_MAX = 70
SIGMA = 0.01   # as the unconstrained Quadrotor case of tests/test_gpu_policy_rollout.py


def c5(lib, batch):
    return configs.quadrotor_problem(batch=batch, N=21, tf=2.5, constrained=True, goal_inds=configs.C5_GOAL_INDS, lib=lib)


@pytest.fixture(scope="module")
def solved(oracle):
    """Quadrotor C5 at B = 3, N = 21, solved by the oracle's ALSolver; gains from the oracle's phase API at the solution (non-zero duals and
    penalties in the expansion); S_MAX perturbed start states and the restatement for them."""
    p = c5(oracle, 3)
    T.ALSolver(p).solve()
    I.expand(p); I.backwardpass(p)
    g = I.gains(p)
    Xbar, Ubar = T.states(p), T.controls(p)
    X0s = R.sample_starts(p, Xbar, SIGMA, S_MAX)
    Xr, Ur, dxr = R.restate(oracle, p, Xbar, Ubar, g["K"], g["d"], X0s)
    Jr, cr = R.oracle_cost_and_violation(oracle, c5, Xr, Ur)
    return SimpleNamespace(p=p, Xbar=Xbar, Ubar=Ubar, K=np.ascontiguousarray(g["K"]), d=np.ascontiguousarray(g["d"]), X0s=X0s, ref=(Xr, Ur, dxr, Jr, cr))


def host_rollout(host, c, S, lane_map=0, chunk=0, trajectories=True):
    p = c.p
    o = T.SolverOptions(lib=p._lib)
    p._call("get_options", C.byref(o._o))
    B, N, n, m = p.B, p.N, p.n, p.m
    x0s = np.ascontiguousarray(c.X0s[:, :S])
    X, U = np.full((B, S, N, n), np.nan), np.full((B, S, N - 1, m), np.nan)
    J, cm, dx = np.zeros((B, S)), np.zeros((B, S)), np.zeros((B, S))
    st, kl = np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32)
    pd = lambda a: a.ctypes.data_as(PD)
    rc = host.policy_host_rollout(C.addressof(p._desc), C.addressof(o._o), S, lane_map, chunk, pd(np.ascontiguousarray(c.Xbar)), pd(np.ascontiguousarray(c.Ubar)),
                                  pd(c.K), pd(c.d), pd(x0s), 0.0, None, None, None, pd(X) if trajectories else None, pd(U) if trajectories else None,
                                  pd(J), pd(cm), pd(dx), st.ctypes.data_as(PI), kl.ctypes.data_as(PI))
    assert rc == 0, host.policy_host_last_error()
    return SimpleNamespace(X=X if trajectories else None, U=U if trajectories else None, J=J, c_max=cm, dx_max=dx, status=st, k_limit=kl)


def test_the_reference_is_not_vacuous(solved):
    """Checked on the reference alone: no sample leaves the limits (status 0 is then what the kernel must report), and the violation is
    positive on at least 90 % of the perturbed samples (sample 0 of each trajectory is the nominal start)."""
    Xr, Ur, dxr, Jr, cr = solved.ref
    o = T.SolverOptions(lib=solved.p._lib)
    solved.p._call("get_options", C.byref(o._o))
    assert np.isfinite(Xr).all() and np.abs(Xr).max() <= o.max_state_value and np.abs(Ur).max() <= o.max_control_value
    perturbed = cr[:, 1:]
    print(f"c_max of the reference: positive on {np.mean(perturbed > 0):.3f} of the perturbed samples, median {np.median(perturbed):.2e}, "
          f"nominal {cr[:, 0]}; dx_max up to {dxr.max():.2e}")
    assert np.mean(perturbed > 0) >= 0.9
    assert dxr[:, 1:].min() > 0


@pytest.mark.parametrize("S", S_VALUES)
def test_constrained_quadrotor_matches_the_restatement(S, host, solved):
    r = host_rollout(host, solved, S)
    R.compare(f"host quadrotor C5 S={S}", r, R.ref_slice(solved.ref, S))
    s_only = host_rollout(host, solved, S, trajectories=False)          # the summary-only call: the same numbers, bit for bit
    for k in ("J", "c_max", "dx_max", "status", "k_limit"):
        np.testing.assert_array_equal(getattr(s_only, k), getattr(r, k), err_msg=k)
    one_wave = host_rollout(host, solved, S, chunk=1)                   # ... and chunks of one wave
    for k in ("X", "U", "J", "c_max", "dx_max", "status", "k_limit"):
        np.testing.assert_array_equal(getattr(one_wave, k), getattr(r, k), err_msg=k)


def test_lane_maps_agree_on_the_constrained_quadrotor(host, solved):
    """At S = 64 either map can serve; at S = 3 the uniform map spends a wave per trajectory: all meet the restatement."""
    r = host_rollout(host, solved, 64, lane_map=1)
    R.compare("host quadrotor C5 S=64 packed", r, R.ref_slice(solved.ref, 64))
    r = host_rollout(host, solved, 3, lane_map=2)
    R.compare("host quadrotor C5 S=3 uniform", r, R.ref_slice(solved.ref, 3))
