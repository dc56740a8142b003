"""The scan backward pass's element arithmetic on the host (csrc/scan_combine.h compiled by g++ through tests/host_shim): the value-only
form of the combination — what the last scan round computes — gives the bytes of the full form's (eta, J); combine(identity, identity)
is the identity's bytes (the condition under which a lane past lane 63's reach may read lane 63 as it is); and the trimmed round loop
on a simulated wave matches the untrimmed one for every block count.  Stand-alone program, also under ASan + UBSan."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
SHIM = ROOT / "tests" / "host_shim"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", *SAN]], ids=["plain", "asan_ubsan"])
def test_scan_combine_harness(flags, tmp_path):
    exe = tmp_path / "scan_combine_harness"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "scan_combine_harness.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1500:])
    words = r.stdout.split()
    assert int(words[words.index("fails") + 1]) == 0 and int(words[words.index("checks") + 1]) > 30000, r.stdout[-500:]


def test_the_kernel_uses_the_header_the_harness_compiles():
    """k_scan.h takes ScanEl / scan_lu_solve / scan_combine from scan_combine.h and keeps no copy; the header has no lane intrinsics."""
    kernel, header = (CSRC / "k_scan.h").read_text(), (CSRC / "scan_combine.h").read_text()
    assert '#include "scan_combine.h"' in kernel
    for name in ("struct ScanEl", "void scan_lu_solve(", "void scan_combine("):
        assert name in header and name not in kernel, name
    for word in ("__shfl", "ds_bpermute", "__ballot", "threadIdx", "__builtin_amdgcn_"):
        assert word not in header, word
