#!/usr/bin/env python3
"""Records tests/golden/cw_parent_bits.npz: what handles on the general kernel variants compute WITHOUT per-trajectory cost weights — the
fixture of tests/test_gpu_cost_weights_unflagged.py.  Run it on an MI355X against the library of the commit to pin
(TRAJOPT_HIP_LIBRARY=<that build's libtrajopt_hip.so>); the solves are those of tests/cw_parent_cases.py.

Usage: tools/cw_parent_bits.py [out.npz]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import trajopt_amd as T  # noqa: E402
import cw_parent_cases as P  # noqa: E402


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "cw_parent_bits.npz"
    lib = T.load_hip_library()
    data = {"build_id": np.array(lib.build_id())}
    for name in P.CASES:
        data.update(P.run(name, lib))
        print(name, "iterations", int(data[f"{name}_iterations"].sum()), "status", np.unique(data[f"{name}_status"]))
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({out.stat().st_size} bytes) from build {lib.build_id()}")


if __name__ == "__main__":
    main()
