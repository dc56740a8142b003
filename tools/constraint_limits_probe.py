#!/usr/bin/env python3
"""What per-trajectory constraint limits cost (to_set_constraint_limits_batch).

The same AL solve (constraint_tolerance = 1e-4) — Cartpole constrained, B = 1024, N = 101, and the Quadrotor with the C5 constraint set,
B = 8192, N = 201 — timed twice on one handle configuration each: with the shared limits (the default path: tuned kernel variants, the
control-block constraints cached in registers), and with B copies of those same limits set per trajectory (the general variants, the
flagged constraint read per trajectory through the descriptor-table path).  Same problem, same limits, so the iteration counts should agree
and the difference is the cost of the routing and of the per-lane loads, not of another problem.  Run the script on the parent commit's
library as well (TRAJOPT_HIP_LIBRARY names it; it then prints the shared row only): that row is the yardstick and shows whether the default
path moved; run it there twice in the same session for the run-to-run spread.

Every figure is the mean of --reps solves after one untimed warm-up solve of the same handle configuration; each solve runs on a fresh
handle (a solve starts from the handle's trajectory) and is timed by the library's own device-side span (solve_ms) next to the host wall
clock around the blocking call.  Prints one JSON line per measurement and a markdown table.

Usage: tools/constraint_limits_probe.py [--reps 3] [--models cartpole,quadrotor]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import trajopt_amd as T  # noqa: E402
from trajectoryoptimization_jl_amd import configs  # noqa: E402

BUILD = {"cartpole": lambda: configs.cartpole_problem(batch=1024, N=101, tf=5.0, constrained=True),
         "quadrotor": lambda: configs.quadrotor_problem(batch=8192, N=201, tf=5.0, constrained=True, goal_inds=configs.C5_GOAL_INDS)}


def one_solve(name, per_trajectory):
    p = BUILD[name]()
    if per_trajectory:
        T.set_constraint_limits_batch(p, 0, T.get_constraint_limits_batch(p, 0))    # B copies of the descriptor's own limits
    info = np.zeros(8, np.int32)
    p._call("solver_path", p._pi(info))
    t = time.perf_counter()
    s = T.ALSolver(p, constraint_tolerance=1e-4).solve()
    wall = (time.perf_counter() - t) * 1e3
    return dict(wall_ms=wall, solve_ms=float(s.solve_ms), iterations=int(s.total_iterations), batch_steps=int(s.batch_steps),
                succeeded=float(np.mean(s.stats["status"] == T.capi.SOLVE_SUCCEEDED)), path=[int(v) for v in info], B=p.B, N=p.N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", default="cartpole,quadrotor")
    a = ap.parse_args()
    lib = T.load_hip_library()
    have = "set_constraint_limits_batch" in lib._fn
    rows = []
    for name in a.models.split(","):
        for per_trajectory in ((False, True) if have else (False,)):
            one_solve(name, per_trajectory)  # warm-up, untimed
            runs = [one_solve(name, per_trajectory) for _ in range(a.reps)]
            r = dict(build=lib.build_id(), model=name, B=runs[0]["B"], N=runs[0]["N"], limits="per trajectory" if per_trajectory else "shared",
                     solve_ms=round(float(np.mean([x["solve_ms"] for x in runs])), 3), wall_ms=round(float(np.mean([x["wall_ms"] for x in runs])), 3),
                     runs_solve_ms=[round(x["solve_ms"], 3) for x in runs], iterations=runs[0]["iterations"], batch_steps=runs[0]["batch_steps"],
                     succeeded=runs[0]["succeeded"], path=runs[0]["path"])
            r["trajectory_iterations_per_s"] = round(r["iterations"] / (r["solve_ms"] * 1e-3))
            rows.append(r)
            print(json.dumps(r), flush=True)
    print("\nbuild %s\n\n| model | B | N | limits | solve ms (mean of %d) | runs | wall ms | iterations | batch steps | M trajectory-iterations/s | to_solver_path |"
          "\n|---|---|---|---|---|---|---|---|---|---|---|" % (lib.build_id(), a.reps))
    for r in rows:
        print(f"| {r['model']} | {r['B']} | {r['N']} | {r['limits']} | {r['solve_ms']} | {r['runs_solve_ms']} | {r['wall_ms']} | {r['iterations']} | {r['batch_steps']} | "
              f"{r['trajectory_iterations_per_s'] / 1e6:.3f} | {r['path']} |")


if __name__ == "__main__":
    main()
