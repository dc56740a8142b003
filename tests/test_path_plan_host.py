"""Kernel-path selection (csrc/path_plan.h: plan_paths at to_create, plan_step per batch step, path_report behind to_solver_path, forward_mode,
compact_grid) compiled for the HOST.  tests/host_shim/path_plan_harness.cpp holds (a) pinned rows — the to_solver_path report and the plan
fields at 256 compute units, derived by hand from the to_create / to_solver_path that held this logic before it moved into that header — for
the BASELINE configurations, Cartpole batches on either side of the lane / scan / two-launch thresholds, the double integrators, the hybrid
and model-vector traits and every knob flipped once; (b) invariants over every model's traits x batch sizes x constraints x cost blocks x
every knob at its extreme values: one backward flavour, fused kernels only where compiled, wave shapes within 64 lanes, and — for every active
count 0 .. B of the batch (plans with at most one knob set; pairs of knobs and the working sets a repacking solve moves into: a stride plus both
sides of every threshold) — the blocks each forward launch touches (two-launch line search included) inside what the plan allocated; the report agrees with the step plan; forward_mode never names a variant that is not compiled;
compact_grid covers every batch up to its limit.  (c) the harness counts what it reached: every step kind and every branch on both sides."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_path_plan(tmp_path):
    exe = tmp_path / "path_plan_harness"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", str(ROOT / "trajectoryoptimization.jl_amd" / "csrc"),
                    str(ROOT / "tests" / "host_shim" / "path_plan_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-6000:]
    words = r.stdout.split()
    count = lambda k: int(words[words.index(k) + 1])
    assert count("fails") == 0
    assert count("rows") >= 60 and count("plans") > 100000 and count("steps") > 10 ** 8 and count("checks") > 10 ** 6, r.stdout
    # both sides of every decision were reached
    for k in ("split", "fused_lane", "fused_coop", "scan", "base_shape", "deep_shape", "one_wave", "two_wave", "store_x", "controls_only",
              "one_launch", "two_launch"):
        assert count(k) > 10000, (k, r.stdout)
    for k in ("scan_below_max", "scan_above_max", "forward_found", "forward_none", "compact_one", "compact_two", "compact_refused"):
        assert count(k) > 50, (k, r.stdout)
