"""List mode of the two-wave forward pass (csrc/fwd_list.h, path_plan.h solve_forward_list) on the HOST: the rank a scan wave computes for
its trajectory from the batch's active flags — passes of 64 flags as ballots, walked in chunks as k_scan.h walks them — against a plain
loop, for Bp = 64, 128, 1024, 2048, full and ragged batches (1, 17, 65, 200, Bp - 1, Bp - 63) and the flag patterns all / none / one /
alternating / a random third / two thirds; the list all the waves write together against the plain compaction; every flag load inside
the array; the forward pass's grid; and which solves run in the mode.  The harness has its own main and runs a second time built with
-fsanitize=address,undefined (host code only)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_rank_list_and_mode_decision(sanitize, tmp_path):
    exe = tmp_path / "fwd_list_harness"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-I", str(ROOT / "tests" / "host_shim"), "-I", str(ROOT / "trajectoryoptimization.jl_amd" / "csrc"),
                    str(ROOT / "tests" / "host_shim" / "fwd_list_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    words = r.stdout.split()
    assert int(words[words.index("batches") + 1]) >= 4 * 4 * 7 and int(words[words.index("ranks") + 1]) > 10000, r.stdout
    assert int(words[words.index("fails") + 1]) == 0
