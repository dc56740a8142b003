"""The solves behind tests/golden/cw_parent_bits.npz (tools/cw_parent_bits.py records them, tests/test_gpu_cost_weights_unflagged.py holds
every later build to them bit for bit): handles that run the GENERAL kernel variants and never call to_set_cost_weights_batch.  They were
recorded on an MI355X from the library of the commit before per-trajectory cost weights existed; the general variants are the ones a
handle with weights runs, so they are the ones the feature could have disturbed.

  gl        Cartpole N = 41, B = 70, one goal per trajectory (to_set_cost_linear_batch), iLQR
  cl        constrained Cartpole N = 41, B = 70, one control bound per trajectory (to_set_constraint_limits_batch), ALTRO
  nonsel    Cartpole N = 41, B = 70 with a quadratic-form NormConstraint on the control (a non-selector constraint) and the goal, AL
  pm        Cartpole N = 41, B = 70, one plant per trajectory (to_set_model_params_batch), iLQR
  quad_gl   Quadrotor N = 31, B = 24, one goal position per trajectory, iLQR
"""
import math

import numpy as np

import trajopt_amd as T
from trajectoryoptimization_jl_amd import configs

B, N, TF = 70, 41, 2.0
QB, QN, QTF = 24, 31, 1.0
STAT_KEYS = ("status", "iterations", "iterations_outer", "iterations_pn", "cost", "c_max")
AL_KW = dict(constraint_tolerance=1e-4)
# X and U are kept for these trajectories (the head of the first tile, its tail and the whole partial second tile); the stats — the cost to
# the last bit among them — for every trajectory
KEEP = np.r_[0:12, 56:70]
QKEEP = np.r_[0:24:2]


def cartpole_goals(batch, seed=205):
    rng = np.random.default_rng(seed)
    Xf = np.tile([0.0, math.pi, 0.0, 0.0], (batch, 1))
    Xf[:, 0] += rng.uniform(-0.4, 0.4, batch)
    return Xf


def quadrotor_goals(batch, seed=206):
    th = math.radians(135.0) / 2
    Xf = np.tile(np.r_[2.0, 3.0, 1.0, math.cos(th), 0.0, 0.0, math.sin(th), np.zeros(6)], (batch, 1))
    Xf[:, :3] += np.random.default_rng(seed).uniform(-0.5, 0.5, (batch, 3))
    return Xf


def cartpole_models(batch, seed=207, spread=0.2):
    s = 1.0 + spread * np.random.default_rng(seed).uniform(-1.0, 1.0, (batch, 3))
    models = [T.Cartpole(mc=1.0 * a, mp=0.2 * b, l=0.5 * c) for a, b, c in s]
    models[0] = T.Cartpole()
    return models


def _gl(lib):
    p = configs.cartpole_problem(batch=B, N=N, tf=TF, lib=lib)
    T.set_goal_state(p, cartpole_goals(B))
    return p, T.iLQRSolver(p)


def _cl(lib):
    p = configs.cartpole_problem(batch=B, N=N, tf=TF, constrained=True, u_bnd=10.0, lib=lib)
    u = np.random.default_rng(208).uniform(8.0, 12.0, (B, 1))
    T.set_bounds_batch(p, 0, u_max=u, u_min=-u)
    return p, T.ALTROSolver(p)


def _nonsel(lib):
    p0 = configs.cartpole_problem(batch=1, N=N, tf=TF, lib=lib)
    n, m = p0.n, p0.m
    cons = T.ConstraintList(n, m, N)
    T.add_constraint(cons, T.NormConstraint(n, m, 10.0, T.Inequality(), "control"), range(1, N))
    T.add_constraint(cons, T.GoalConstraint(p0.xf), N)
    p = T.Problem(p0.model, p0.obj, np.zeros(n), TF, xf=p0.xf, constraints=cons, batch=B, lib=lib)
    p.set_initial_state(configs.cartpole_x0(B))
    T.initial_controls(p, np.full(m, 0.01))
    return p, T.ALSolver(p, **AL_KW)


def _pm(lib):
    p = configs.cartpole_problem(batch=B, N=N, tf=TF, lib=lib)
    T.set_model_params(p, cartpole_models(B))
    return p, T.iLQRSolver(p)


def _quad_gl(lib):
    p = configs.quadrotor_problem(batch=QB, N=QN, tf=QTF, lib=lib)
    T.set_goal_state(p, quadrotor_goals(QB))
    return p, T.iLQRSolver(p)


CASES = {"gl": _gl, "cl": _cl, "nonsel": _nonsel, "pm": _pm, "quad_gl": _quad_gl}


def run(name, lib):
    """-> {key: array} of one case: the stats of STAT_KEYS, X and U."""
    p, solver = CASES[name](lib)
    s = solver.solve()
    out = {f"{name}_{k}": s.stats[k].copy() for k in STAT_KEYS}
    keep = QKEEP if name.startswith("quad") else KEEP
    out[f"{name}_X"], out[f"{name}_U"] = T.states(p)[keep], T.controls(p)[keep]
    return out
