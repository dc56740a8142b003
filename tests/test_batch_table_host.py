"""The one host routine behind every per-trajectory table with a spare tile (csrc/desc_lower.h tile_rows: DevProblem::pm, dtb, cl, gw, ga),
without a GPU: tests/host_shim/batch_table_harness.cpp, a program of its own, checks it lane by lane — live entries at the address the kernels
form, the padding lanes of the last tile and the whole spare tile on the shared row, the length, the round trip, values == NULL — over a grid
of (L, B), checks the images of pm and cl as the library builds them, and prints a hash of all five images for fixed inputs.  PARENT holds the
hashes of the same inputs recorded from the five loops the routine replaced (dtb, gw, ga: the functions desc_lower.h had; pm, cl: the loops of
upload_plants and upload_constraint_limits in trajopt_hip.hip, transcribed): the images are byte-identical."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
SHIM = ROOT / "tests" / "host_shim"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]

# FNV-1a (64 bit) over the bytes of each image, B = 1, 64, 65, 300
PARENT = {
    "pm": {1: "5c524fefd17d9b57", 64: "fa221f1736e9a788", 65: "ea7ed3a940e6604b", 300: "d0e49df95ef20c89"},
    "cl": {1: "ca40843dabe47be5", 64: "875075cfc393626d", 65: "9501c27b97f4cebd", 300: "6888525867fbf842"},
    "dtb": {1: "37df9cd95d05d758", 64: "5c0066ab1018755e", 65: "f3b460b05becca39", 300: "8e8c1b7e22465fa6"},
    "gw": {1: "a252f44eb90e7819", 64: "1dba7ded4a966a65", 65: "1c9a923a678fef05", 300: "f86a509e54a02c71"},
    "ga": {1: "005299bdadddc9f4", 64: "075778257606e308", 65: "38b2c1fe6edf206c", 300: "c9680142f316bdf8"},
}


def _harness(tmp_path, flags=()):
    exe = tmp_path / "batch_table_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", *flags, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "batch_table_harness.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-3000:], r.stderr[-1500:])
    return r.stdout


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    return _harness(tmp_path_factory.mktemp("batch_table"))


def _hashes(out):
    got = {}
    for m in re.finditer(r"^hash (\w+) (\d+) ([0-9a-f]{16})$", out, flags=re.M):
        got.setdefault(m.group(1), {})[int(m.group(2))] = m.group(3)
    return got


def test_every_lane_of_every_image(harness_out):
    words = harness_out.split()
    # 32 grid cases, each entry of each image twice (values, NULL), then pm and cl at B = 65
    assert int(words[words.index("checks") + 1]) > 2 * 10 ** 5 and int(words[words.index("fails") + 1]) == 0


def test_harness_under_asan_ubsan(tmp_path):
    assert _hashes(_harness(tmp_path, SAN)) == PARENT


@pytest.mark.parametrize("B", [1, 64, 65, 300])
@pytest.mark.parametrize("table", ["pm", "cl", "dtb", "gw", "ga"])
def test_image_is_byte_identical_to_the_replaced_loop(harness_out, table, B):
    assert _hashes(harness_out)[table][B] == PARENT[table][B]


def test_one_tiling_loop_in_the_library():
    """The loop shape — tiles, rows, 64 lanes, `t * 64 + l` — stands once in csrc, and trajopt_hip.hip sizes no spare tile of its own."""
    hits = [f.name for f in sorted(CSRC.iterdir()) if f.suffix in (".h", ".hip") and "t * 64 + l" in f.read_text()]
    assert hits == ["desc_lower.h"] and (CSRC / "desc_lower.h").read_text().count("t * 64 + l") == 1
    assert "/ 64 + 1" not in (CSRC / "trajopt_hip.hip").read_text()
