#!/usr/bin/env python3
"""Records tests/golden/pm_only_parent.npz: what handles with to_set_model_params_batch ALONE compute — the fixture of
tests/test_gpu_time_steps.py::test_plants_only_handle_computes_what_it_did_before_time_steps_existed.  Run it on an MI355X against the
library of the commit to pin (TRAJOPT_HIP_LIBRARY=<that build's libtrajopt_hip.so>); the fleets are those of
tests/test_gpu_model_params_batch.py (Cartpole iLQR seed 11, constrained Cartpole ALTRO seed 14, Quadrotor iLQR seed 15; B = 70).

Usage: tools/pm_only_golden.py [out.npz]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import trajopt_amd as T  # noqa: E402
import model_params_fleet as M  # noqa: E402

CASES = (("cartpole", "cartpole", 11, "ilqr", 70), ("altro", "cartpole_con", 14, "altro", 70), ("quadrotor", "quadrotor", 15, "ilqr", 16))


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "pm_only_parent.npz"
    lib = T.load_hip_library()
    data = {"build_id": np.array(lib.build_id())}
    for name, kind, seed, solver, keep in CASES:
        p = M.build(kind, lib, 70)
        T.set_model_params(p, M.draw_models(kind, 70, seed))
        s = M.SOLVERS[solver](p).solve()
        for k in ("status", "iterations", "cost", "c_max", "iterations_pn"):
            data[f"{name}_{k}"] = s.stats[k].copy()
        data[f"{name}_X"], data[f"{name}_U"] = T.states(p)[:keep], T.controls(p)[:keep]
    np.savez_compressed(out, **data)
    print(f"wrote {out} ({out.stat().st_size} bytes) from build {lib.build_id()}")


if __name__ == "__main__":
    main()
