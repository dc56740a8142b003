"""Reference for per-trajectory time steps (tests/test_gpu_time_steps.py, tests/test_time_steps_oracle.py): B single-trajectory ORACLE
problems, problem b built with ``dt = dt_b`` (its own final time ``t0 + sum(dt_b)``) and — through ``batch=1, b_offset=b`` — with trajectory
b's own start state: the scheme of tests/model_params_fleet.py, whose ``build`` makes the configurations.  The oracle knows nothing about
per-trajectory steps and is not changed.  A fleet is computed once per configuration and shared by the tests that need it; nothing in it is
modified afterwards.

Step fleets, drawn by a seeded generator:
  uniform  tf_b within +-25 % of the configuration's tf (trajectory 0 keeps it), uniform steps (tf_b - t0) / (N - 1) — the expression
           ``Problem`` forms for its own uniform step, so oracle problem b is simply built with ``tf = tf_b``;
  ragged   dt_b[k] = h_b (1 + 0.2 u_bk), u uniform in [-1, 1], h_b the uniform step of a tf_b drawn as above: another grid per trajectory AND
           per knot, so that a kernel that reads dt[0], the neighbour knot or the lane's step instead of the trajectory's shows up.

Vetted on the oracle alone before the seeds were fixed (tests/test_time_steps_oracle.py repeats it): share of SOLVE_SUCCEEDED per fleet in
SOLVES below — cartpole_coop 100 % / 100 % (ragged / uniform), cartpole_lane 100 % / 100 %, dint_al_bounds 100 % / 100 %,
cartpole_altro 100 % / 100 %, quadrotor_mfma 100 % / 100 %; plants + steps 100 %, bounds + steps 100 %."""
import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
import model_params_fleet as M

SPREAD_TF = 0.25
SPREAD_KNOT = 0.2
KEYS = ("iterations", "iterations_outer", "iterations_pn", "status", "cost", "c_max")
# the configuration's (N, tf) per kind, as model_params_fleet.build defaults them
SHAPES = {"cartpole": (31, 1.5), "cartpole_con": (51, 2.5), "quadrotor": (41, 1.0), "quadrotor_con": (31, 2.5), "dint": (31, 3.0)}


def shape_of(kind, N=None, tf=None):
    n0, t0 = SHAPES[kind]
    return N or n0, tf or t0


def draw_final_times(tf, B, seed):
    """[B] final times within +-25 % of tf; trajectory 0 keeps tf."""
    t = tf * (1.0 + SPREAD_TF * np.random.default_rng(seed).uniform(-1.0, 1.0, B))
    t[0] = tf
    return t


def draw_steps(tf, N, B, seed, ragged):
    """[B, N-1] time steps of a fleet (t0 = 0)."""
    t = draw_final_times(tf, B, seed)
    h = np.repeat(((t - 0.0) / (N - 1))[:, None], N - 1, axis=1)     # the expression of Problem's own uniform step
    if ragged:
        h = h * (1.0 + SPREAD_KNOT * np.random.default_rng(seed + 1000).uniform(-1.0, 1.0, (B, N - 1)))
    return h


def with_steps(p, dt, lib, options=None):
    """Problem ``p`` (batch 1 or B) rebuilt on ``lib`` with the time steps ``dt`` [N-1] in its descriptor — tf = t0 + sum(dt) — and p's start
    states and controls."""
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    kw = {"options": T.SolverOptions(lib=lib, **options)} if options else {}
    q = T.Problem(p.model, p.obj, T.get_initial_state(p)[0], p.t0 + float(dt.sum()), xf=None if np.all(np.isnan(p.xf)) else p.xf,
                  constraints=p.constraints, t0=p.t0, dt=dt, integration=p.integration, batch=p.B, lib=lib, **kw)
    q.set_initial_state(T.get_initial_state(p))
    T.initial_controls(q, T.controls(p))
    return q


def dint_bounds_problem(lib, batch, b_offset=0, u_max=1.5, u_min=-1.5, N=31, tf=3.0, dt=None):
    """model_params_fleet's ``dint`` (D = 2, |u| <= 1.5 on knots 1 .. N-1) with the control bound given: per-trajectory limits on the GPU
    handle, the trajectory's own in the descriptor of its oracle problem."""
    D, n, m = 2, 4, 2
    xf = np.r_[1.0 * np.arange(1, D + 1), np.zeros(D)]
    obj = T.LQRObjective(np.ones(n), 0.1 * np.ones(m), 100 * np.ones(n), xf, N)
    cons = T.ConstraintList(n, m, N)
    T.add_constraint(cons, T.BoundConstraint(n, m, u_max=u_max, u_min=u_min), (1, N - 1))
    p = T.Problem(T.DoubleIntegrator(1.0, D), obj, np.zeros(n), tf if dt is None else float(np.sum(dt)), xf=xf, constraints=cons, batch=batch, lib=lib,
                  dt=None if dt is None else np.ascontiguousarray(dt, dtype=np.float64))
    b = np.arange(b_offset, b_offset + batch, dtype=np.uint64)
    X0 = np.zeros((batch, n))
    from trajectoryoptimization_jl_amd import configs
    for j in range(D):
        X0[:, j] = configs.splitmix64_uniform(7, np.uint64(D) * b + np.uint64(j)) - 0.5
    p.set_initial_state(X0)
    return p


def draw_bounds(B, seed):
    """[B] control bounds within +-20 % of 1.5 (trajectory 0 keeps 1.5): u_max = -u_min = a_b for both controls."""
    a = 1.5 * (1.0 + 0.2 * np.random.default_rng(seed).uniform(-1.0, 1.0, B))
    a[0] = 1.5
    return a


class StepFleet:
    """Results of B single-trajectory oracle problems with their own time steps, stacked along the batch axis (the attributes of
    model_params_fleet.Fleet).  ``dt``: [B, N-1]; ``tfs``: [B] for a uniform fleet (problem b is then built with tf = tfs[b], no dt);
    ``models``: one model per trajectory (plants + steps); ``bounds``: [B] control bounds of ``dint`` (limits + steps)."""

    def __init__(self, kind, oracle, dt, tfs=None, solver=None, phases=False, x0=None, models=None, bounds=None, solver_kw=None, **kw):
        B = len(dt)
        self.B, self.dt = B, dt
        self.stats = {k: [] for k in KEYS}
        rows = {k: [] for k in ("X", "U", "Xr", "J", "Jk", "F", "A", "Bm", "K", "d", "ls", "Jn", "defect")}
        for b in range(B):
            model = None if models is None else models[b]
            if bounds is not None:
                p = dint_bounds_problem(oracle, 1, b_offset=b, u_max=bounds[b], u_min=-bounds[b], dt=None if tfs is not None else dt[b],
                                        **({"tf": float(tfs[b])} if tfs is not None else {}), **kw)
            elif tfs is not None:
                p = M.build(kind, oracle, 1, b_offset=b, model=model, x0=x0, **{**kw, "tf": float(tfs[b])})
            else:
                p = with_steps(M.build(kind, oracle, 1, b_offset=b, model=model, x0=x0, **kw), dt[b], oracle, options=kw.get("options"))
            if phases:
                T.rollout(p)
                rows["Xr"].append(T.states(p)[0]); rows["J"].append(T.cost(p)[0]); rows["Jk"].append(T.stage_costs(p)[0])
                rows["F"].append(I.discrete_jacobian(p)[0])
                rows["defect"].append(T.dynamics_defect(p)[0])
                I.expand(p)
                A, Bm = I.dynamics_jacobians(p)
                rows["A"].append(A[0]); rows["Bm"].append(Bm[0])
                I.backwardpass(p)
                g = I.gains(p)
                rows["K"].append(g["K"][0]); rows["d"].append(g["d"][0])
                ls, Jn = I.forwardpass(p)
                rows["ls"].append(ls[0]); rows["Jn"].append(Jn[0])
            if solver:
                s = M.SOLVERS[solver](p, **(solver_kw or {})).solve()
                for k in KEYS:
                    self.stats[k].append(s.stats[k][0])
                rows["X"].append(T.states(p)[0]); rows["U"].append(T.controls(p)[0])
        self.stats = {k: np.array(v) for k, v in self.stats.items() if v}
        for k, v in rows.items():
            if v:
                setattr(self, k, np.array(v))


# ------------------------------------------------------------------------------------------------ the named fleets
DT_COST = dict(cost_dt_scaling=1)  # stage costs x dt: the cost kernels read the step too (value, expansion, the polish's metric)
#          kind            B    seed  solver   environment                     to_solver_path()[0] (0 cooperative, 1 MFMA, 2 lane)   options
SOLVES = {
    "cartpole_coop": ("cartpole", 70, 111, "ilqr", {}, 0, None),
    "cartpole_lane": ("cartpole", 300, 112, "ilqr", {"TRAJOPT_BACKWARD": "lane"}, 2, DT_COST),
    "dint_al_bounds": ("dint", 70, 113, "al", {}, 0, DT_COST),
    "cartpole_altro": ("cartpole_con", 70, 114, "altro", {}, 0, DT_COST),
    "quadrotor_mfma": ("quadrotor", 70, 115, "ilqr", {}, 1, None),
}
PHASES = {"cartpole": 121, "quadrotor": 122}     # ragged, B = 70, N = 41, tf = 1.0
# Stage costs x dt on the Cartpole only.  Vetted on the oracle alone: a 1e-12 relative nudge of the control guess moves the oracle's own J_new of
# the Cartpole fleet by 1e-14 either way, of the Quadrotor fleet by 3e-12 with plain costs — and by 1.1e-10 .. 1.7e-10 with stage costs x dt
# (seeds 122 .. 125 alike: the stage weights fall to 1/40 of a terminal weight 100 times theirs), above the 1e-10 its J_new is held to.
PHASE_KW = {"cartpole": dict(N=41, tf=1.0, options=DT_COST), "quadrotor": dict(N=41, tf=1.0)}
PLANTS_STEPS = ("cartpole", 70, 131, "ilqr")     # own plants AND own (ragged) steps
BOUNDS_STEPS = ("dint", 70, 132, "al")           # own control bounds AND own (ragged) steps
POLICY = ("cartpole", 70, 141)
ORDER = {"cartpole": 151, "quadrotor": 152}
_cache = {}


def okw(options):
    return {"options": options} if options else {}


def steps_of(kind, B, seed, ragged, N=None, tf=None, **_):
    N, tf = shape_of(kind, N, tf)
    return draw_steps(tf, N, B, seed, ragged), draw_final_times(tf, B, seed)


def solve_fleet(case, oracle, ragged):
    kind, B, seed, solver, _, _, options = SOLVES[case]
    key = ("solve", case, ragged)
    if key not in _cache:
        dt, tf = steps_of(kind, B, seed, ragged)
        _cache[key] = StepFleet(kind, oracle, dt, tfs=None if ragged else tf, solver=solver, **okw(options))
    return _cache[key]


def phase_fleet(kind, oracle):
    key = ("phases", kind)
    if key not in _cache:
        dt, _ = steps_of(kind, 70, PHASES[kind], True, **PHASE_KW[kind])
        _cache[key] = StepFleet(kind, oracle, dt, phases=True, **PHASE_KW[kind])
    return _cache[key]


def plants_steps_fleet(oracle):
    kind, B, seed, solver = PLANTS_STEPS
    if "plants" not in _cache:
        dt, _ = steps_of(kind, B, seed, True)
        models = M.draw_models(kind, B, seed)
        _cache["plants"] = (StepFleet(kind, oracle, dt, solver=solver, models=models), models)
    return _cache["plants"]


def bounds_steps_fleet(oracle):
    kind, B, seed, solver = BOUNDS_STEPS
    if "bounds" not in _cache:
        dt, _ = steps_of(kind, B, seed, True)
        a = draw_bounds(B, seed)
        _cache["bounds"] = (StepFleet(kind, oracle, dt, solver=solver, bounds=a), a)
    return _cache["bounds"]
