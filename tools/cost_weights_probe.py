#!/usr/bin/env python3
"""What per-trajectory cost weights cost (to_set_cost_weights_batch).

The same iLQR solve — Cartpole B = 1024, N = 101 and Quadrotor B = 4096, N = 201, the BASELINE shapes — on ONE handle, without weights (the
default path: scan / fused / packed kernels, the stage cost preloaded) and with every cost's weights set to B copies of its descriptor's
own diagonal (the general variants, the weights read per trajectory from DevProblem::gw, the stage cost read per knot).  Same problem, same
weights, so the iteration counts agree and the difference is the cost of the routing and of the per-lane loads, not of another problem.
Each configuration: one untimed solve, then --reps timed solves from the same start (solve_ms: the library's device-side span), then one
solve with the hipEvent profile on for the per-phase kernel times (to_get_profile: expansion, backward pass, forward pass, polish).  On a
library without the entry points (the parent commit, via TRAJOPT_HIP_LIBRARY) it prints the shared rows alone — the yardstick.
Prints one JSON line per measurement and a markdown table.

Usage: tools/cost_weights_probe.py [--reps 3] [--models cartpole,quadrotor]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import trajopt_amd as T  # noqa: E402
from trajectoryoptimization_jl_amd import configs  # noqa: E402

BUILD = {"cartpole": (lambda: configs.cartpole_problem(batch=1024, N=101, tf=5.0), lambda p: np.full(p.m, 0.01)),
         "quadrotor": (lambda: configs.quadrotor_problem(batch=4096, N=201, tf=5.0), lambda p: T.Quadrotor().hover_control())}


def solve(p, u0, profile=False):
    T.initial_controls(p, u0)
    T.rollout(p)
    if profile:
        p._call("reset_profile"); p._call("set_profiling", 1)
    t = time.perf_counter()
    s = T.iLQRSolver(p).solve()
    wall = (time.perf_counter() - t) * 1e3
    out = dict(wall_ms=wall, solve_ms=float(s.solve_ms), iterations=int(s.total_iterations), batch_steps=int(s.batch_steps),
               succeeded=float(np.mean(s.stats["status"] == T.capi.SOLVE_SUCCEEDED)))
    if profile:
        p._call("set_profiling", 0)
        ms, ln = (C.c_double * 4)(), (C.c_int64 * 4)()
        p._call("get_profile", ms, ln)
        out["phase_ms"] = [round(v, 3) for v in ms]; out["phase_launches"] = list(ln)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", default="cartpole,quadrotor")
    a = ap.parse_args()
    lib = T.load_hip_library()
    have = "set_cost_weights_batch" in lib._fn
    rows = []
    for name in a.models.split(","):
        build, guess = BUILD[name]
        p = build()
        u0 = guess(p)
        for weights in ((False, True) if have else (False,)):
            if weights:
                for ci in range(len(p._cost_objs)):
                    T.set_cost_weights_batch(p, ci, *T.get_cost_weights_batch(p, ci))     # B copies of the descriptor's own diagonal
            info = np.zeros(8, np.int32)
            p._call("solver_path", p._pi(info))
            solve(p, u0)  # untimed
            runs = [solve(p, u0) for _ in range(a.reps)]
            prof = solve(p, u0, profile=True)
            r = dict(build=lib.build_id(), model=name, B=p.B, N=p.N, weights="per trajectory" if weights else "shared",
                     solve_ms=round(float(np.mean([x["solve_ms"] for x in runs])), 3), wall_ms=round(float(np.mean([x["wall_ms"] for x in runs])), 3),
                     runs_solve_ms=[round(x["solve_ms"], 3) for x in runs], iterations=runs[0]["iterations"], batch_steps=runs[0]["batch_steps"],
                     succeeded=runs[0]["succeeded"], path=[int(v) for v in info], phase_ms=prof["phase_ms"], phase_launches=prof["phase_launches"])
            r["trajectory_iterations_per_s"] = round(r["iterations"] / (r["solve_ms"] * 1e-3))
            rows.append(r)
            print(json.dumps(r), flush=True)
    print("\nbuild %s\n\n| model | B | N | weights | solve ms (mean of %d) | runs | iterations | batch steps | M trajectory-iterations/s | to_solver_path | "
          "expansion / backward / forward / polish ms (launches) |\n|---|---|---|---|---|---|---|---|---|---|---|" % (lib.build_id(), a.reps))
    for r in rows:
        ph = " / ".join(f"{m} ({n})" for m, n in zip(r["phase_ms"], r["phase_launches"]))
        print(f"| {r['model']} | {r['B']} | {r['N']} | {r['weights']} | {r['solve_ms']} | {r['runs_solve_ms']} | {r['iterations']} | {r['batch_steps']} | "
              f"{r['trajectory_iterations_per_s'] / 1e6:.3f} | {r['path']} | {ph} |")


if __name__ == "__main__":
    main()
