#!/usr/bin/env python3
"""Closed-loop policy rollout (to_policy_rollout) against the open-loop rollout, and its two lane maps against each other.

For the Cartpole at N = 101 and the Quadrotor at N = 201 (the BASELINE horizons), with LANES = B * S samples in flight:
  * wall time of the summary-only call (no trajectories, refresh_gains = 0) as (B = LANES / 64, S = 64) — the uniform lane map — and as
    (B = LANES, S = 1) — the packed map —, next to T.rollout (the open-loop kernel, one lane per trajectory) at B = LANES;
  * at S = 64, the uniform map against the per-lane body forced onto the same samples (TRAJOPT_POLICY_MAP=packed);
  * the stochastic call (to_policy_rollout_mc) at the same shapes under the default lane map: process noise (w), plus measurement noise
    (w+v), plus one plant per sample (w+v+plants: the planning model's parameters, copied per sample).  Its yardstick is the noise-free
    row of the same shape; the cost of the noise is the difference.
Every figure is the mean of REPS timed calls after one warm call (host wall clock around the blocking C call: upload of the start states,
kernel, download of the five per-sample arrays).  The gains are those of one backward pass at the initial guess; start states are the
nominal start plus 0.01 N(0, 1).  Prints one JSON line per measurement and a markdown table.

Usage: tools/policy_rollout_probe.py [--lanes 65536] [--reps 3] [--models cartpole,quadrotor]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import trajopt_amd as T  # noqa: E402
from trajopt_amd import internal as I  # noqa: E402
from trajectoryoptimization_jl_amd import configs  # noqa: E402

BUILD = {"cartpole": lambda B: configs.cartpole_problem(batch=B, N=101, tf=5.0),
         "quadrotor": lambda B: configs.quadrotor_problem(batch=B, N=201, tf=5.0)}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return float(np.mean(ts)), ts


def starts(p, S, seed=1):
    x0 = T.states(p)[:, None, 0, :]
    X0s = x0 + 0.01 * np.random.default_rng(seed).standard_normal((p.B, S, p.n))
    if p.n == 13:
        X0s[..., 3:7] /= np.linalg.norm(X0s[..., 3:7], axis=-1, keepdims=True)
    return np.ascontiguousarray(X0s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", default="cartpole,quadrotor")
    a = ap.parse_args()
    rows = []

    def record(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)
    for name in a.models.split(","):
        for B, S in ((a.lanes // 64, 64), (a.lanes, 1)):
            p = BUILD[name](B)
            T.rollout(p); I.expand(p); I.backwardpass(p)
            X0s = starts(p, S)
            maps = ("uniform", "packed") if S == 64 else ("packed",)
            for lane_map in maps:
                os.environ["TRAJOPT_POLICY_MAP"] = lane_map
                ms, ts = timed(lambda: T.policy_rollout(p, X0s, refresh_gains=False), a.reps)
                r = T.policy_rollout(p, X0s, refresh_gains=False)
                record(model=name, N=p.N, what="policy_rollout", B=B, S=S, lane_map=lane_map, ms=round(ms, 3), runs=[round(t, 3) for t in ts],
                       completed=float(np.mean(r.status == 0)))
            os.environ.pop("TRAJOPT_POLICY_MAP")
            plants = np.zeros((B, S, 16))
            plants[..., :len(p.model.params())] = p.model.params()
            sg = 0.01 if name == "cartpole" else 0.002
            for what, kw in (("w", dict(noise=T.PolicyNoise(1, sigma_w=sg))), ("w+v", dict(noise=T.PolicyNoise(1, sigma_w=sg, sigma_v=sg))),
                             ("w+v+plants", dict(noise=T.PolicyNoise(1, sigma_w=sg, sigma_v=sg), plants=plants))):
                ms, ts = timed(lambda: T.policy_rollout(p, X0s, refresh_gains=False, **kw), a.reps)
                r = T.policy_rollout(p, X0s, refresh_gains=False, **kw)
                record(model=name, N=p.N, what=f"policy_rollout {what}", B=B, S=S, lane_map="default", ms=round(ms, 3), runs=[round(t, 3) for t in ts],
                       completed=float(np.mean(r.status == 0)))
            if S == 1:
                ms, ts = timed(lambda: T.rollout(p), a.reps)
                record(model=name, N=p.N, what="rollout (open loop)", B=B, S=1, lane_map="-", ms=round(ms, 3), runs=[round(t, 3) for t in ts], completed=1.0)
            del p
    print("\n| model | N | call | B | S | lane map | ms (mean of %d) |\n|---|---|---|---|---|---|---|" % a.reps)
    for r in rows:
        print(f"| {r['model']} | {r['N']} | {r['what']} | {r['B']} | {r['S']} | {r['lane_map']} | {r['ms']} |")


if __name__ == "__main__":
    main()
