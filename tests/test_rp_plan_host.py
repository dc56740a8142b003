"""The re-use decision of the repacked working sets (csrc/rp_plan.h, called by rp_move) compiled for the HOST and replayed over every
sequence of one, two and three differently configured solves on one handle: every table of carried arrays a handle can produce (per-trajectory
cost terms on/off x constraints on/off x per-trajectory constraint parameters on/off, at the dimensions of the Cartpole, double-integrator and
hybrid problems) in every order, with first moves that shrink, stay and grow, for both working sets.  The harness keeps its own ledger of
allocated bytes: every array and the map must fit the buffer they get, and no buffer is re-used across a changed kind or row length.
(With the rule reduced to "same number of arrays, capacity large enough" the harness fails on the pair  cost terms -> constraint
parameters  of a constrained handle: the buffer sized for the cost terms receives the duals.)"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_rp_plan_reuse_decisions(tmp_path):
    exe = tmp_path / "rp_plan_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "trajectoryoptimization.jl_amd" / "csrc"),
                    str(ROOT / "tests" / "host_shim" / "rp_plan_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    words = r.stdout.split()
    count = lambda k: int(words[words.index(k) + 1])
    assert count("fails") == 0
    assert count("reuse") > 1000 and count("realloc") > 1000, r.stdout      # both decisions were exercised
