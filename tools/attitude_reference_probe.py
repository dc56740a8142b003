#!/usr/bin/env python3
"""What per-trajectory attitude references cost (to_set_cost_attitude_batch / to_set_tracking_attitude).

Solve: the same Quadrotor iLQR solve — B = 4096, N = 201, the C3 shape of BASELINE.md — on ONE handle in three configurations:
  shared     no per-trajectory cost data (the default path: packed expansion, the stage cost preloaded);
  weights    every cost's weights set to B copies of its descriptor's own diagonal (the GW kernel instances; on this build they also load
             the four q_ref values per cost evaluation; on the parent commit, via TRAJOPT_HIP_LIBRARY, they do not: the yardstick);
  attitudes  every cost's q_ref set to B copies of its descriptor's own (the same instances, reached through the new setter).
Same problem, same values, so the iteration counts agree and the differences are the loads.  Each configuration: one untimed solve, then
--reps timed solves from the same start (solve_ms: the library's device-side span), then one solve with the hipEvent profile on for the
per-phase kernel times (expansion, backward pass, forward pass, polish).

Window: a tracking objective of the same shape (one DiagonalQuatCost per knot, Nref = 2 N); the mean wall time of --moves calls of
to_set_tracking_window (4 B bytes up, one launch of k_track_lower, one synchronisation) with attitude tracking off and on, and the bytes the
kernel writes (N (n + m) B 8 for the linear rows, N 4 B 8 more for the attitude rows).

On a library without the entry points it prints the rows it can.  One JSON line per measurement and a markdown table.

Usage: tools/attitude_reference_probe.py [--reps 3] [--moves 20] [--B 4096] [--N 201]"""
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


def tracking_problem(B, N):
    """One DiagonalQuatCost per knot; the reference: hover at a slowly yawing attitude along a straight line, 2 N knots."""
    uh = T.Quadrotor().hover_control()
    Qd, Rd = np.array([10.0, 10, 10, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1]), np.full(4, 1e-2)
    x = np.zeros(13); x[3] = 1.0
    costs = [T.DiagonalQuatCost(Qd * (10.0 if k == N - 1 else 1.0), Rd, -Qd * x, -Rd * uh, 0.0, 1.0, x[3:7], terminal=(k == N - 1)) for k in range(N)]
    p = T.Problem(T.Quadrotor(), T.Objective(costs), np.zeros(13), 5.0, batch=B)
    p.set_initial_state(configs.quadrotor_x0(B, 0))
    T.initial_controls(p, uh)
    Nref = 2 * N
    Xref = np.zeros((B, Nref, 13))
    yaw = 0.01 * np.arange(Nref)[None, :] * (1.0 + np.arange(B)[:, None] / B)
    Xref[:, :, 0] = 0.01 * np.arange(Nref)[None, :]
    Xref[:, :, 3], Xref[:, :, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    return p, Xref, np.tile(uh, (B, Nref, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--N", type=int, default=201)
    a = ap.parse_args()
    lib = T.load_hip_library()
    have_w, have_a = "set_cost_weights_batch" in lib._fn, "set_cost_attitude_batch" in lib._fn
    rows = []
    u0 = T.Quadrotor().hover_control()
    for cfg in ("shared",) + (("weights",) if have_w else ()) + (("attitudes",) if have_a else ()):
        p = configs.quadrotor_problem(batch=a.B, N=a.N, tf=5.0)
        for ci in range(len(p._cost_objs)):
            if cfg == "weights":
                T.set_cost_weights_batch(p, ci, *T.get_cost_weights_batch(p, ci))       # B copies of the descriptor's own diagonal
            elif cfg == "attitudes":
                T.set_cost_attitude_batch(p, ci, T.get_cost_attitude_batch(p, ci))      # B copies of the descriptor's own q_ref
        info = np.zeros(8, np.int32)
        p._call("solver_path", p._pi(info))
        solve(p, u0)  # untimed
        runs = [solve(p, u0) for _ in range(a.reps)]
        prof = solve(p, u0, profile=True)
        r = dict(build=lib.build_id(), what="solve", B=p.B, N=p.N, config=cfg, solve_ms=round(float(np.mean([x["solve_ms"] for x in runs])), 3),
                 runs_solve_ms=[round(x["solve_ms"], 3) for x in runs], iterations=runs[0]["iterations"], batch_steps=runs[0]["batch_steps"],
                 succeeded=runs[0]["succeeded"], path=[int(v) for v in info], phase_ms=prof["phase_ms"], phase_launches=prof["phase_launches"])
        rows.append(r)
        print(json.dumps(r), flush=True)
    moves = []
    if "set_tracking_reference_batch" in lib._fn:
        p, Xref, Uref = tracking_problem(a.B, a.N)
        T.set_tracking_reference_batch(p, Xref, Uref, start=1, end="hold")
        for att in ((False, True) if have_a else (False,)):
            if att:
                T.set_tracking_attitude(p, True)
            T.set_tracking_window(p, 2)  # untimed
            t = time.perf_counter()
            for i in range(a.moves):
                T.set_tracking_window(p, 3 + i)
            ms = (time.perf_counter() - t) * 1e3 / a.moves
            r = dict(build=lib.build_id(), what="window", B=p.B, N=p.N, attitude=att, window_call_ms=round(ms, 4),
                     bytes_written=p.N * (p.n + p.m) * p.B * 8 + (p.N * 4 * p.B * 8 if att else 0))
            moves.append(r)
            print(json.dumps(r), flush=True)
    print("\nbuild %s\n\n| config | B | N | solve ms (mean of %d) | runs | iterations | batch steps | to_solver_path | expansion / backward / forward / polish ms (launches) |\n"
          "|---|---|---|---|---|---|---|---|---|" % (lib.build_id(), a.reps))
    for r in rows:
        ph = " / ".join(f"{m} ({n})" for m, n in zip(r["phase_ms"], r["phase_launches"]))
        print(f"| {r['config']} | {r['B']} | {r['N']} | {r['solve_ms']} | {r['runs_solve_ms']} | {r['iterations']} | {r['batch_steps']} | {r['path']} | {ph} |")
    print("\n| window move | B | N | ms per to_set_tracking_window | bytes written by k_track_lower |\n|---|---|---|---|---|")
    for r in moves:
        print(f"| attitude {'on' if r['attitude'] else 'off'} | {r['B']} | {r['N']} | {r['window_call_ms']} | {r['bytes_written']} |")


if __name__ == "__main__":
    main()
