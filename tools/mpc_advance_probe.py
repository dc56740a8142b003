#!/usr/bin/env python3
"""What one MPC period costs through to_mpc_advance and through the host recipe it replaces.

Shapes: C2 (Cartpole N = 101) at B = 1024 and B = 32 768, C3 (Quadrotor N = 201) at B = 4096.  Every handle first gets a 5-iteration iLQR
solve (a plan and its gains), then runs MPC periods with shift 1.  Three paths, each on a handle of its own, on the same library:

  `recipe`   INTEGRATION.md's host composition: T.policy_rollout(prob, x_meas[:, None, :], trajectories=True) — the whole closed-loop
             trajectory transposed and downloaded in chunks — the shift in numpy, set_initial_state, initial_controls, T.rollout
  `advance`  T.mpc_advance(prob, x_meas): the same measured state uploaded, the trajectory stays on the device
  `resident` T.mpc_advance(prob): no measured state either — the handle's own x0, the form mpc_run uses from the second period on

Two figures per path: the advance alone, and the advance plus the 5-iteration iLQR re-solve that follows it (one MPC period).  Each is the
mean of --reps timed periods after one untimed warm period; host wall clock around the blocking calls (every entry point synchronises the
handle's stream before it returns).  The measured state of a period is the state the previous period arrived at, kept on the host.

Prints one JSON line per (shape, path) and, with --out, writes the markdown table (profiles/mpc_advance.md).

Usage: tools/mpc_advance_probe.py [--reps 3] [--out table.md] [--shapes cartpole_C2_1024,cartpole_C2_32768,quadrotor_C3_4096]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import trajopt_amd as T  # noqa: E402
from trajectoryoptimization_jl_amd import configs  # noqa: E402

SHAPES = {"cartpole_C2_1024": lambda: configs.cartpole_problem(batch=1024, N=101, tf=5.0),
          "cartpole_C2_32768": lambda: configs.cartpole_problem(batch=32768, N=101, tf=5.0),
          "quadrotor_C3_4096": lambda: configs.quadrotor_problem(batch=4096, N=201, tf=5.0)}
PATHS = ("recipe", "advance", "resident")
SHIFT = 1


def shift(U, s):
    return np.concatenate([U[:, s:], np.repeat(U[:, -1:], s, axis=1)], axis=1)


def step(p, path, x_meas):
    """One advance; returns the state it arrived at."""
    if path == "recipe":
        r = T.policy_rollout(p, np.ascontiguousarray(x_meas[:, None, :]), trajectories=True)
        x_next = np.ascontiguousarray(r.X[:, 0, SHIFT])
        p.set_initial_state(x_next)
        T.initial_controls(p, shift(r.U[:, 0], SHIFT))
        T.rollout(p)
        return x_next
    return T.mpc_advance(p, x_meas if path == "advance" else None, shift=SHIFT).x_next


def measure(name, path, reps):
    p = SHAPES[name]()
    s = T.iLQRSolver(p, iterations=5)
    s.solve()
    x = T.get_initial_state(p)
    adv, period, its = [], [], 0
    for rep in range(reps + 1):                 # period 0 is the warm one
        t0 = time.perf_counter()
        x = step(p, path, x)
        t1 = time.perf_counter()
        s.solve()
        t2 = time.perf_counter()
        if rep:
            adv.append((t1 - t0) * 1e3)
            period.append((t2 - t0) * 1e3)
            its += int(s.total_iterations)
    return dict(case=name, B=p.B, N=p.N, path=path, advance_ms=round(float(np.mean(adv)), 3), period_ms=round(float(np.mean(period)), 3),
                runs_advance_ms=[round(v, 3) for v in adv], runs_period_ms=[round(v, 3) for v in period], resolve_iterations=its,
                checksum=float(np.abs(x).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    lib = T.load_hip_library()
    rows = []
    for name in a.shapes.split(","):
        for path in PATHS:
            r = dict(build=lib.build_id(), **measure(name, path, a.reps))
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        lines = [f"# One MPC period: to_mpc_advance and the host recipe (library build {lib.build_id()})", "",
                 f"`tools/mpc_advance_probe.py --reps {a.reps}`: shift {SHIFT}, mean of {a.reps} timed periods after one warm period, host wall clock in ms.",
                 "`advance`: the step alone; `period`: the step plus the 5-iteration iLQR re-solve that follows it.", "",
                 "| shape | B | N | path | advance ms | period ms | advance runs | period runs |", "|---|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['case']} | {r['B']} | {r['N']} | {r['path']} | {r['advance_ms']} | {r['period_ms']} | {r['runs_advance_ms']} | {r['runs_period_ms']} |")
        lines += ["", "Ratios, recipe / path (above 1: the path is faster than the recipe):", "", "| shape | path | advance | period |", "|---|---|---|---|"]
        for r in rows:
            if r["path"] == "recipe":
                base = r
                continue
            lines.append(f"| {r['case']} | {r['path']} | {base['advance_ms'] / r['advance_ms']:.2f} | {base['period_ms'] / r['period_ms']:.2f} |")
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
