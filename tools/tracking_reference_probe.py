#!/usr/bin/env python3
"""What moving every trajectory's tracking window costs through to_set_tracking_window and through the host recipe it replaces.

Shape: C2 as a tracking problem — Cartpole, N = 101, B = 1024, one DiagonalCost per knot, a sinusoidal reference of Nref = 200 knots and a
window start per trajectory.  Two paths, each on a handle of its own:

  `recipe`  N calls of to_set_cost_linear_batch, q_b = -Q x_ref[j], r_b = -R u_ref[j] computed in numpy, each call staged through the host
  `window`  one to_set_tracking_window: 4 B bytes up, one launch of k_track_lower

Each figure is the mean of --reps timed moves after one untimed warm move, host wall clock around the blocking calls (every entry point
synchronises the handle's stream before it returns); every move shifts every start by one knot.  A library without the feature (an older
build named by TRAJOPT_HIP_LIBRARY) runs the recipe alone.  Both paths end on the same terms (checksum of the solve that follows).

The kernel's own time is not a host clock's business: run the probe under `rocprofv3 --kernel-trace --stats` with `--paths window` and read
k_track_lower from the statistics; the bytes it must move are N (n + m) B doubles read and as many written (--bytes prints them).

Prints one JSON line per path and, with --out, writes the markdown table.

Usage: tools/tracking_reference_probe.py [--reps 10] [--paths recipe,window] [--out table.md]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import trajopt_amd as T  # noqa: E402

N, B, NREF, TF = 101, 1024, 200, 5.0


def problem():
    model = T.Cartpole()
    Q, R, Qf = np.array([10.0, 1.0, 1.0, 1.0]), np.array([0.1]), np.array([100.0, 10.0, 10.0, 10.0])
    obj = T.TrackingObjective(Q, R, np.zeros((4, N)), np.zeros((1, N - 1)), Qf)
    p = T.Problem(model, obj, np.zeros(4), TF, batch=B)
    T.initial_controls(p, np.zeros(1))
    return p


def reference():
    b = np.arange(B)
    A, w = 0.3 + 0.1 * (b % 7), 1.0 + 0.3 * ((b // 7) % 10)
    t = (TF / (N - 1)) * np.arange(NREF)[None, :]
    X, U = np.zeros((B, NREF, 4)), np.zeros((B, NREF, 1))
    X[:, :, 0], X[:, :, 2] = A[:, None] * np.sin(w[:, None] * t), (A * w)[:, None] * np.cos(w[:, None] * t)
    U[:, :, 0] = -1.5 * (A * w * w)[:, None] * np.sin(w[:, None] * t)
    return X, U, (1 + (3 * b) % 50).astype(np.int32)


def feed_by_recipe(p, X, U, start):
    rows = np.arange(B)
    for k in range(N):
        j = np.minimum(start.astype(np.int64) - 1 + k, NREF - 1)
        cid = int(p._cost_index[k])
        c = p._cost_objs[cid]
        q, r = np.ascontiguousarray(-(c.Q[None, :] * X[rows, j])), np.ascontiguousarray(-(c.R[None, :] * U[rows, j]))
        p._call("set_cost_linear_batch", cid, p._pd(q), p._pd(r))


def measure(path, reps):
    p = problem()
    X, U, start = reference()
    if path == "window":
        T.set_tracking_reference_batch(p, X, U, start, end="hold")
    ms = []
    for rep in range(reps + 1):                 # move 0 is the warm one
        s = (start + rep + 1).astype(np.int32)
        t0 = time.perf_counter()
        if path == "window":
            T.set_tracking_window(p, s)
        else:
            feed_by_recipe(p, X, U, s)
        t1 = time.perf_counter()
        if rep:
            ms.append((t1 - t0) * 1e3)
    sol = T.iLQRSolver(p, iterations=5).solve()
    return dict(path=path, B=B, N=N, Nref=NREF, move_ms=round(float(np.mean(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4),
                reps=reps, checksum=float(np.abs(T.states(p)).sum()), iterations=int(sol.total_iterations))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--paths", default="recipe,window")
    ap.add_argument("--out", default="")
    ap.add_argument("--bytes", action="store_true")
    a = ap.parse_args()
    lib = T.load_hip_library()
    moved = 2 * N * 5 * B * 8
    if a.bytes:
        print(json.dumps(dict(kernel_bytes=moved, read=moved // 2, written=moved // 2)))
    rows = []
    for path in a.paths.split(","):
        if path == "window" and "set_tracking_window" not in lib._fn:
            print(json.dumps(dict(path=path, skipped="the library does not export to_set_tracking_window")), flush=True)
            continue
        r = dict(build=lib.build_id(), **measure(path, a.reps))
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        lines = [f"`tools/tracking_reference_probe.py --reps {a.reps}` (library build {lib.build_id()}): Cartpole, N = {N}, B = {B}, Nref = {NREF}; one move of every",
                 "trajectory's window, host wall clock in ms, mean / min / max of the timed moves after one warm move.", "",
                 "| path | move ms | min | max | checksum of the following solve |", "|---|---|---|---|---|"]
        lines += [f"| {r['path']} | {r['move_ms']} | {r['min_ms']} | {r['max_ms']} | {r['checksum']!r} ({r['iterations']} iterations) |" for r in rows]
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
