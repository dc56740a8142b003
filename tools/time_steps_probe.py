#!/usr/bin/env python3
"""What planning on one set of time steps per trajectory costs (to_set_time_steps_batch).

The same iLQR solve — the C2-shaped Cartpole and the C3-shaped Quadrotor, at the shapes of tests/test_gpu_time_steps.py (B = 70) and at the
BASELINE batch sizes (B = 1024, N = 101 and B = 4096, N = 201) — on one library, three ways: `shared` (the default path: scan / fused /
packed kernels), `plants` (to_set_model_params_batch with B copies of the shared model: the flagged general instances) and `steps`
(to_set_time_steps_batch with the descriptor's own steps: the same instances, now reading the step per trajectory).  Same problem, same
numbers, so the iteration counts agree and the difference is the cost of the path.  Run it on the parent commit's library as well
(TRAJOPT_HIP_LIBRARY=...; it has no `steps` row): its `plants` row is the comparison line for this library's `steps` row.

Every figure is the mean of --reps solves after one untimed warm-up solve of the same configuration; each solve runs on a fresh handle and
is timed by the library's own device-side span (solve_ms) next to the host wall clock around the blocking call.  Prints one JSON line per
measurement.

Usage: tools/time_steps_probe.py [--reps 3] [--tag name]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import trajopt_amd as T  # noqa: E402
from trajectoryoptimization_jl_amd import configs  # noqa: E402

BUILD = {"cartpole_test": lambda: configs.cartpole_problem(batch=70, N=31, tf=1.5),
         "quadrotor_test": lambda: configs.quadrotor_problem(batch=70, N=41, tf=1.0),
         "cartpole_C2": lambda: configs.cartpole_problem(batch=1024, N=101, tf=5.0),
         "quadrotor_C3": lambda: configs.quadrotor_problem(batch=4096, N=201, tf=5.0)}


def one_solve(name, mode):
    p = BUILD[name]()
    if mode == "plants":
        pp = np.zeros((p.B, 16))
        q = p.model.params()
        pp[:, : len(q)] = q
        T.set_model_params(p, pp)
    elif mode == "steps":
        T.set_time_steps_batch(p, T.time_steps(p))
    info = np.zeros(8, np.int32)
    p._call("solver_path", p._pi(info))
    t = time.perf_counter()
    s = T.iLQRSolver(p).solve()
    wall = (time.perf_counter() - t) * 1e3
    return dict(wall_ms=wall, solve_ms=float(s.solve_ms), iterations=int(s.total_iterations), batch_steps=int(s.batch_steps),
                succeeded=float(np.mean(s.stats["status"] == T.capi.SOLVE_SUCCEEDED)), path=[int(v) for v in info], B=p.B, N=p.N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    lib = T.load_hip_library()
    modes = ["shared", "plants"] + (["steps"] if "set_time_steps_batch" in lib._fn else [])
    for name in BUILD:
        for mode in modes:
            one_solve(name, mode)  # warm-up, untimed
            runs = [one_solve(name, mode) for _ in range(a.reps)]
            r = dict(tag=a.tag, build=lib.build_id(), case=name, B=runs[0]["B"], N=runs[0]["N"], mode=mode,
                     solve_ms=round(float(np.mean([x["solve_ms"] for x in runs])), 3), wall_ms=round(float(np.mean([x["wall_ms"] for x in runs])), 3),
                     runs_solve_ms=[round(x["solve_ms"], 3) for x in runs], iterations=runs[0]["iterations"], batch_steps=runs[0]["batch_steps"],
                     succeeded=runs[0]["succeeded"], path=runs[0]["path"])
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
