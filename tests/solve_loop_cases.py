"""The solves behind tests/golden/solve_loop_parent.json (tools/solve_loop_parent.py records them, tests/test_gpu_solve_loop.py holds every later
build to them entry for entry): what the HOST loop of a solve did, read from the library's own TRAJOPT_SYNC_DEBUG=1 trace on stderr.  They were
recorded on an MI355X from the library of the commit before the loop's decisions moved into csrc/solve_loop.h.

  repack   tests/repack_cases.py cartpole_duals at B = 200 with the recipe of tests/test_gpu_repack_small.py (fused lane path, a set of any size
           moves as soon as a tenth of it has finished): iLQR, dual update, iLQR — the second solve drains through both working sets
  altro    constrained Quadrotor N = 61, B = 150 (the shape of test_gpu_pn.py::test_polish_in_workspace_chunks) under ALTRO with the early polish
           armed: up to four hand-overs, the first when half the batch is left
  list     the smallest Cartpole iLQR solve of tests/test_gpu_forward_list.py, list mode of the two-wave forward pass switched on

Per solve: every "[sync-debug] step" line as [step, B, Bp, level, the active count the step was planned with], every "rp_move ... after
k_repack_move" line as [level, count, B, Bp], batch_steps, and the iterations and status arrays."""
import re

import trajopt_amd as T
from trajectoryoptimization_jl_amd import configs
import repack_cases as R

STEP = re.compile(r"\[sync-debug\] step (\d+) B=(\d+) Bp=(\d+) level=(\d+) store_x-path=(\d+): (.*)")
MOVE = re.compile(r"\[sync-debug\] rp_move level (\d+) -> \d+ count (\d+) \(B (\d+) Bp (\d+), cap \d+ / \d+\) after k_repack_move: (.*)")
LIST_B, LIST_N = 1, 21

# what each case sets before its handle is made (the knobs of a handle's path are read by to_create, the switches of the loop by every solve)
ENV = {
    "repack": {"TRAJOPT_BACKWARD": "lane", "TRAJOPT_REPACK_AT": "0.9", "TRAJOPT_GUARD": "0", "TRAJOPT_REPACK": "1"},
    "altro": {"TRAJOPT_PN_EARLY": "4", "TRAJOPT_PN_EARLY_AT": "2"},
    "list": {"TRAJOPT_FWD_LIST": "1"},
}


def _entry(err, stats, batch_steps):
    steps, moves = list(STEP.finditer(err)), list(MOVE.finditer(err))
    assert steps and all(m.group(6) == "no error" for m in steps) and all(m.group(5) == "no error" for m in moves), err[-2000:]
    return {"steps": [[int(v) for v in m.groups()[:5]] for m in steps], "moves": [[int(v) for v in m.groups()[:4]] for m in moves],
            "batch_steps": int(batch_steps), "iterations": [int(v) for v in stats["iterations"]], "status": [int(v) for v in stats["status"]]}


def _repack(lib, take):
    c = R.CASES["cartpole_duals"](lib, 200)
    out = []
    R.run(c, lambda k, snap: out.append(_entry(take(), snap.stats, snap.batch_steps)))
    return out


def _altro(lib, take):
    p = configs.quadrotor_problem(batch=150, N=61, tf=3.0, constrained=True, goal_inds=configs.C5_GOAL_INDS, lib=lib)
    s = T.ALTROSolver(p, n_steps=configs.C5_PN_STEPS).solve()
    return [_entry(take(), s.stats, s.batch_steps)]


def _list(lib, take):
    p = configs.cartpole_problem(batch=LIST_B, N=LIST_N, tf=0.05 * (LIST_N - 1), lib=lib)
    s = T.iLQRSolver(p, iterations=25).solve()
    return [_entry(take(), s.stats, s.batch_steps)]


CASES = {"repack": _repack, "altro": _altro, "list": _list}


def run(name, lib, setenv, take):
    """-> one entry per solve of the case.  setenv(name, value) sets an environment variable of this process (the caller puts it back);
    take() -> what the C library has written to stderr since the last call."""
    for k, v in ENV[name].items():
        setenv(k, v)
    setenv("TRAJOPT_SYNC_DEBUG", "1")
    take()
    return CASES[name](lib, take)


def is_real(name, solves):
    """The recorded solve is a real one: more than 90 % of the trajectories SOLVE_SUCCEEDED, more than one chunk of batch steps, and in the
    repack case at least three moves.  Of the repack recipe that is the LAST solve, the one that reads per-trajectory duals (as in
    tests/test_gpu_repack_small.py); the iLQR solve before the dual update is recorded and compared too, whatever its iteration cap leaves."""
    s = solves[-1]
    ok = sum(v == T.capi.SOLVE_SUCCEEDED for v in s["status"])
    real = ok > 0.9 * len(s["status"]) and s["batch_steps"] > R.CHECK_EVERY
    return real and all(len(e["steps"]) >= e["batch_steps"] for e in solves) and (name != "repack" or len(s["moves"]) >= 3)
