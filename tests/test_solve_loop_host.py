"""The host loop of every solve (csrc/solve_loop.h: SolveLoop, read_solve_knobs), without a GPU.

tests/host_shim/solve_loop_harness.cpp compiles the driver with g++ as a stand-alone program under AddressSanitizer + UBSan (nothing is loaded
into python) and plays the device: per-step active counts from per-trajectory iteration counts, a configuration, and the move that finds no
memory.  (a) The trace of the driver — every operation with its arguments — equals the trace of the loop solve_impl had before the driver
existed, which the harness keeps verbatim; (b) the moves equal repack_cases.predicted_moves, the model the GPU trace is held to
(tests/test_gpu_repack_small.py); (c) invariants of the driver's trace alone; (d) what the randomized cases reached."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import repack_cases as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
SRC = ROOT / "tests" / "host_shim" / "solve_loop_harness.cpp"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("solve_loop") / "solve_loop_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(CSRC), str(SRC), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def report(harness):
    r = subprocess.run([str(harness)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    out = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[-1] == ";":
            out[w[0]] = {int(v) for v in w[1:-1]}
        else:
            out.update({k: int(v) for k, v in zip(w[0::2], w[1::2])})
    return out


def test_driver_equals_the_parent_loop_and_keeps_its_invariants(report):
    """(a) and (c): one comparison of whole traces per case, and the invariants of every record."""
    assert report["fails"] == 0
    assert report["cases"] >= 10 ** 5 and report["checks"] > 10 * report["cases"]


def test_randomized_cases_reach_every_path(report):
    """(d)"""
    assert report["max_steps_seen"] == {1, 2, 3, 4, 5, 8, 9, 81, 301}
    assert {1, 63, 64, 65, 200} <= report["batches_seen"]
    assert {5, 50, 95} <= report["rp_at_percent_seen"] and len(report["rp_at_percent_seen"]) >= 10 and min(report["rp_at_percent_seen"]) == 5 \
        and max(report["rp_at_percent_seen"]) == 95
    assert {0, 1, 4, 8} <= report["early_seen"] and {1, 2, 4} <= report["early_div_seen"]
    for key in ("repack_on", "repack_off", "mode_al", "mode_ilqr", "declined_first", "declined_middle", "declined_last", "solves_that_moved",
                "op_step", "op_copy", "op_wait", "op_drain", "op_consume", "op_publish", "op_move", "op_moved", "op_snapshot", "op_polish", "op_end",
                "end_first_step", "end_mid_chunk", "end_chunk_edge", "end_max_steps", "end_in_drain"):
        assert report.get(key, 0) >= 50, (key, report.get(key))
    assert report["op_end"] == report["cases"]


def _moves(harness, tmp_path, cases):
    """cases: [(iterations, B, at, rp_min, cap)] -> the accepted moves [(level, count)] of each, from the driver."""
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{cap + 1} {B} 0 {int(rp_min > 0)} {at!r} {rp_min} 0 4 -1 {len(it)} " + " ".join(str(int(i)) for i in it) + "\n"
                            for it, B, at, rp_min, cap in cases))
    r = subprocess.run([str(harness), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("moves")]
    assert len(lines) == len(cases)
    return [list(zip(map(int, w[0::2]), map(int, w[1::2]))) for w in lines]


def test_moves_equal_the_model_on_the_repack_cases(harness, tmp_path, oracle):
    """(b) on the iteration counts of every solve of every case of tests/repack_cases.py at B = 200 (the oracle's: what
    tests/test_repack_cases_oracle.py chooses seeds with), at the knobs of tests/test_gpu_repack_small.py."""
    B, at, rp_min = 200, 0.9, 1
    its = [s.stats["iterations"] for name in R.CASES for s in R.reference(name, B, oracle)]
    got = _moves(harness, tmp_path, [(it, B, at, rp_min, R.CAP) for it in its])
    want = [R.predicted_moves(it, B, at, rp_min) for it in its]
    assert got == want
    assert sum(len(m) >= 3 for m in want) >= len(R.CASES)


def test_moves_equal_the_model_on_drawn_iteration_counts(harness, tmp_path):
    """(b) on drawn iteration counts: batches around the tile size, thresholds across 0.05 .. 0.95, minimum sizes, short and long caps."""
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(400):
        B = int(rng.choice([1, 63, 64, 65, 130, 200]))
        cap = int(rng.choice([3, 8, 25, 80]))
        it = np.minimum(rng.geometric(rng.choice([0.05, 0.2, 0.5]), B) + int(rng.integers(0, 3)), int(rng.choice([cap, cap + 5])))
        cases.append((it, B, float(rng.choice([0.05, 0.3, 0.7, 0.9, 0.95])), int(rng.choice([0, 1, 16, 64])), cap))
    cases.append((np.full(200, 7), 200, 0.9, 1, R.CAP))
    cases.append((np.r_[np.full(100, 3), np.full(100, 40)], 200, 0.9, 1, R.CAP))
    got = _moves(harness, tmp_path, cases)
    want = [R.predicted_moves(*c) for c in cases]
    assert got == want
    assert want[-2:] == [[], [(0, 100)]] and sum(bool(m) for m in want) > 50 and sum(len(m) >= 3 for m in want) > 10
