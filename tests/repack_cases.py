"""The cases of tests/test_gpu_repack_small.py (the repacked working set at small batch: csrc/trajopt_hip.hip rp_setup / rp_move / rp_finish,
csrc/k_generic.h k_repack_*), vetted on the CPU by tests/test_repack_cases_oracle.py.  One builder per case, ``case(lib, B)`` -> Built: the
configured problem, what was set on it per trajectory, and the solve recipe (``run``).  Every trajectory has its own start state;
``only=b`` builds trajectory b of the batch of B alone, with ITS limit,
goal and target in the descriptors (what the oracle, which shares every limit among the trajectories of a problem, is given), and
``shared=True`` the batch with the nominal limit for everybody (what a library that left ``cl`` behind would solve).

  case            model                  constraints                          carried beyond X, U, x0
  cartpole_plain  Cartpole               none                                 -
  cartpole_gl     Cartpole               none                                 gl
  cartpole_duals  Cartpole               |u| <= 10, goal                      lam, mu
  cartpole_cl     Cartpole               |u| <= u_b ~ U(7, 13), goal          lam, mu, cl
  cartpole_all    Cartpole               |u| <= u_b, goal at xf_b             gl, lam, mu, cp, cl
  dint1_bound     double integrator D=1  |u| <= 1.5, goal                     lam, mu
  dint2_cl        double integrator D=2  x4 <= v_b, u_min_b <= u <= u_max_b   lam, mu, cl
  hybrid_bound    hybrid (4,2)->(2,1)    bounds on both sides of the jump,    lam, mu    (padding stays exactly 0)
                                         goal at the reduced dimension

Cartpole: N = 41, tf = 2.0, as the large repack tests; the others N = 41 as well.  The cases with per-trajectory duals run a hand-built AL
loop — iLQR, ``I.dual_update``, iLQR: only iLQR solves repack, and the second one reads per-trajectory duals and penalties.  The penalty
starts at PENALTY (the default 1 leaves the controls of an iLQR solve far outside the bound; with these they end within 1e-3 of it).

An unconstrained double integrator is linear-quadratic: iLQR ends after 3 iterations whatever the start, and nothing ever moves.  The D = 1
and the hybrid case therefore keep their bounds and are solved by iLQR on the augmented Lagrangian at a fixed penalty (see
tests/test_repack_cases_oracle.py): the iteration counts spread over 2 .. 66."""
from types import SimpleNamespace

import numpy as np

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs
import constraint_limit_fleets as F
import model_params_fleet as M

N, TF = 41, 2.0
CAP = 80                        # iLQR iterations of every solve (the existing repack tests: 25 .. 80)
PENALTY = 1e3
U_NOMINAL = 10.0
STAT_KEYS = ("iterations", "status", "cost", "dJ", "gradient", "c_max", "iterations_outer", "iterations_pn", "penalty_max")


class Built(SimpleNamespace):
    """p: the problem; recipe: "ilqr" | "al_loop"; kw: solver options; cl / gl / cp: what was set per trajectory ({constraint: [B, q]}, [B, n],
    {constraint: [B, p]}) — empty where nothing was; hybrid: zero-padded knots."""


def _idx(B, only):
    return np.arange(B) if only is None else np.array([only])


def decades(B, seed, lo, hi):
    """[B] factors 10^U(lo, hi), one per GLOBAL trajectory."""
    return 10.0 ** np.random.default_rng(seed).uniform(lo, hi, B)


# ---- Cartpole --------------------------------------------------------------------------------------------------------------------------
def cartpole_x0(B, seed=None, lo=-2.0):
    """configs.cartpole_x0 (hanging, cart and pole displaced); with ``seed``: moved towards the upright goal by 10^U(lo, 0) per trajectory."""
    x0 = configs.cartpole_x0(B)
    if seed is None:
        return x0
    xf = np.array([0.0, np.pi, 0.0, 0.0])
    return xf + decades(B, seed, lo, 0.0)[:, None] * (x0 - xf)


CARTPOLE_PLAIN_SEED, CARTPOLE_GL_SEED, CARTPOLE_GOALS_SEED = 3, 4, 21


def _cartpole(lib, B, only, constrained, x0, u_max=U_NOMINAL, u_min=-U_NOMINAL):
    idx = _idx(B, only)
    if constrained:
        p = F.cartpole_problem(lib, len(idx), u_max=u_max, u_min=u_min, N=N, tf=TF)
        for i in range(len(p.constraints)):
            I.set_duals(p, i, mu=PENALTY)
    else:
        p = configs.cartpole_problem(batch=len(idx), N=N, tf=TF, lib=lib)
    p.set_initial_state(x0[idx])
    return p


def cartpole_plain(lib, B, only=None, shared=False):
    return Built(p=_cartpole(lib, B, only, False, cartpole_x0(B, CARTPOLE_PLAIN_SEED)), recipe="ilqr", kw={}, cl={}, gl=None, cp={}, hybrid=False)


def cartpole_goals(B):
    from test_handle_reuse_oracle import cart_goals
    return cart_goals(B, CARTPOLE_GOALS_SEED, -2.0, 0.0)


def cartpole_gl(lib, B, only=None, shared=False):
    p = _cartpole(lib, B, only, False, cartpole_x0(B, CARTPOLE_GL_SEED))
    Xf = cartpole_goals(B)[_idx(B, only)]
    T.set_goal_state(p, Xf)
    return Built(p=p, recipe="ilqr", kw={}, cl={}, gl=Xf, cp={}, hybrid=False)


def cartpole_duals(lib, B, only=None, shared=False):
    return Built(p=_cartpole(lib, B, only, True, cartpole_x0(B)), recipe="al_loop", kw={}, cl={}, gl=None, cp={}, hybrid=False)


CARTPOLE_CL_SEED, CARTPOLE_ALL_SEED = 51, 52


def cartpole_bounds(B, seed):
    """-> (u_max [B], u_min [B]), drawn separately around the nominal 10: constraint_limit_fleets.cartpole_limits(split=True)."""
    return F.cartpole_limits(B, split=True, seed=seed, lo=7.0, hi=13.0)


def _limited_cartpole(lib, B, only, shared, seed, x0):
    up, dn = cartpole_bounds(B, seed)
    if only is not None:                     # trajectory `only` alone, its limit in the descriptor
        own = (U_NOMINAL, -U_NOMINAL) if shared else (up[only], dn[only])
        return _cartpole(lib, B, only, True, x0, *own), {}
    p = _cartpole(lib, B, None, True, x0)
    if shared:
        return p, {}
    T.set_bounds_batch(p, 0, u_max=up[:, None], u_min=dn[:, None])
    return p, {0: np.stack([up, dn], axis=1)}            # rows [u max, u min]


def cartpole_cl(lib, B, only=None, shared=False):
    p, cl = _limited_cartpole(lib, B, only, shared, CARTPOLE_CL_SEED, cartpole_x0(B))
    return Built(p=p, recipe="al_loop", kw={}, cl=cl, gl=None, cp={}, hybrid=False)


def cartpole_all(lib, B, only=None, shared=False):
    """Limits, goals on the costs and the GoalConstraint's target, all per trajectory, on one handle."""
    p, cl = _limited_cartpole(lib, B, only, shared, CARTPOLE_ALL_SEED, cartpole_x0(B))
    Xf = cartpole_goals(B)[_idx(B, only)]
    if only is None:
        T.set_goal_state(p, Xf)
    else:
        T.set_goal_state(p, Xf[0])
    return Built(p=p, recipe="al_loop", kw={}, cl=cl, gl=Xf, cp={1: Xf.copy()}, hybrid=False)


# ---- double integrators ----------------------------------------------------------------------------------------------------------------
DINT1_SEED, DINT2_SEED, HYBRID_SEED = 61, 62, 63
DINT_TF = 2.0
DINT_PENALTY, HYBRID_PENALTY, HYBRID_TF = 1e2, 1e4, 4.0


def _penalty(p, mu):
    for i in range(len(p.constraints)):
        I.set_duals(p, i, mu=mu)
    return p


def dint1_bound(lib, B, only=None, shared=False):
    """model_params_fleet's dint1_con (|u| <= 1.5, goal [0.5, 0]) from positions in +-3 and velocities in +-2."""
    idx = _idx(B, only)
    p = M.build("dint1_con", lib, len(idx), N=N, tf=DINT_TF)
    rng = np.random.default_rng(DINT1_SEED)
    x0 = rng.uniform(-1.0, 1.0, (B, 2)) * np.array([3.0, 2.0])
    p.set_initial_state(x0[idx])
    return Built(p=_penalty(p, DINT_PENALTY), recipe="ilqr", kw={}, cl={}, gl=None, cp={}, hybrid=False)


def dint2_limits(B):
    """constraint_limit_fleets.dint_limits' velocity and control limits; start positions in +-3 (its own +-0.2 end in a handful of iterations)."""
    v, up, dn, x0 = F.dint_limits(B, seed=DINT2_SEED)
    x0 = x0.copy()
    x0[:, :2] = np.random.default_rng(DINT2_SEED + 100).uniform(-3.0, 3.0, (B, 2))
    return v, up, dn, x0


def dint2_cl(lib, B, only=None, shared=False):
    """constraint_limit_fleets' dint (one BoundConstraint with a state row and control rows, own limits on five of its six rows)."""
    v, up, dn, x0 = dint2_limits(B)
    idx = _idx(B, only)
    cl = {}
    if only is not None and not shared:
        p = F.dint_problem(lib, 1, x0[idx], v=v[only], u_max=up[only], u_min=dn[only], N=N, tf=DINT_TF)
    else:
        p = F.dint_problem(lib, len(idx), x0[idx], N=N, tf=DINT_TF)
        if not shared:
            x_max = np.full((B, 4), np.inf); x_max[:, 3] = v
            T.set_bounds_batch(p, 0, x_max=x_max, u_max=up, u_min=dn)
            cl = {0: np.concatenate([v[:, None], up, np.full((B, 1), -0.5), dn], axis=1)}        # rows [x4 max, u max, x1 min, u min]
    return Built(p=_penalty(p, DINT_PENALTY), recipe="al_loop", kw={}, cl=cl, gl=None, cp={}, hybrid=False)


def hybrid_bound(lib, B, only=None, shared=False):
    """tests/test_hybrid_dims.py hybrid_problem with its bounds on both sides of the jump and its goal at the reduced dimension, the jump in
    the middle of the horizon: 20 steps of (4, 2), the jump map, 19 steps of (2, 1)."""
    from test_hybrid_dims import hybrid_problem
    idx = _idx(B, only)
    p, costs, x0, hyb = hybrid_problem(lib, batch=len(idx), constrained=True, steps_2d=20, N=N, tf=HYBRID_TF)
    X0 = np.random.default_rng(HYBRID_SEED).uniform(-3.0, 3.0, (B, 4))
    p.set_initial_state(X0[idx])
    return Built(p=_penalty(p, HYBRID_PENALTY), recipe="ilqr", kw={}, cl={}, gl=None, cp={}, hybrid=True)


CASES = {f.__name__: f for f in (cartpole_plain, cartpole_gl, cartpole_duals, cartpole_cl, cartpole_all, dint1_bound, dint2_cl, hybrid_bound)}
ORACLE_COMPARED = ("cartpole_cl", "dint2_cl", "cartpole_all")


# ---- the recipe ------------------------------------------------------------------------------------------------------------------------
def snapshot(s, p):
    st = {k: np.array(s.stats[k]).copy() for k in STAT_KEYS}
    return SimpleNamespace(stats=st, X=T.states(p), U=T.controls(p), J=T.cost(p), batch_steps=int(s.batch_steps))


def ls_after(p):
    """One more expansion, backward pass and forward pass on the solved problem: -> (line-search index [B] int32, J_new [B]).  The solve
    interface reports no line-search index; this is the search the solve would run next, on the home arrays (it moves the trajectory: call
    it last)."""
    I.expand(p); I.backwardpass(p)
    return I.forwardpass(p)


def run(c, after_solve=None):
    """The case's recipe on c.p: -> one snapshot per iLQR solve ("ilqr": one; "al_loop": iLQR, dual update, iLQR -> two).  Every solve states
    all its options.  after_solve(k, snapshot): called behind solve k."""
    p = c.p
    s = T.iLQRSolver(p, T.SolverOptions(lib=p._lib, iterations=CAP, **c.kw))
    out = []
    for k in range(2 if c.recipe == "al_loop" else 1):
        if k:
            I.dual_update(p)
        out.append(snapshot(s.solve(), p))
        if after_solve:
            after_solve(k, out[-1])
    return out


def run_singles(case, lib, B, shared=False, nudge=0.0):
    """The recipe on B single-trajectory problems (constraint_limit_fleets.solve_singles' scheme), stacked: -> snapshots like run's."""
    rows = []
    for b in range(B):
        c = case(lib, B, only=b, shared=shared)
        if nudge:
            F.nudged(c.p, nudge)
        rows.append(run(c))
        rows[-1][-1].ls, rows[-1][-1].J_next = ls_after(c.p)
    out = []
    for k in range(len(rows[0])):
        out.append(SimpleNamespace(stats={key: np.concatenate([r[k].stats[key] for r in rows]) for key in rows[0][k].stats},
                                   X=np.concatenate([r[k].X for r in rows]), U=np.concatenate([r[k].U for r in rows]),
                                   J=np.concatenate([r[k].J for r in rows]), batch_steps=max(r[k].batch_steps for r in rows)))
    out[-1].ls, out[-1].J_next = np.concatenate([r[-1].ls for r in rows]), np.concatenate([r[-1].J_next for r in rows])
    return out


_cache = {}


def reference(name, B, lib, shared=False, nudge=0.0):
    """run_singles for an oracle-compared case, run on the batch for the others; computed once per session, never modified."""
    key = (name, B, shared, nudge)
    if key not in _cache:
        _cache[key] = run_singles(CASES[name], lib, B, shared, nudge) if name in ORACLE_COMPARED else run(CASES[name](lib, B))
    return _cache[key]


# ---- what the solve loop does with a draining batch (csrc/trajopt_hip.hip solve_impl) -------------------------------------------------------
CHECK_EVERY = 4


def active_counts(iterations, steps):
    """counter[k]: trajectories still iterating after batch step k (a trajectory that takes i iterations is active in steps 0 .. i-1)."""
    it = np.asarray(iterations)
    return [int((it > k + 1).sum()) for k in range(steps)]


def predicted_moves(iterations, B, at, rp_min, cap=CAP):
    """The moves the solve loop makes for these per-trajectory iteration counts: the host enqueues chunks of CHECK_EVERY batch steps one
    chunk ahead, reads the active counts of a chunk when the next is enqueued, and once a count it has read is <= at x (size of the set) it
    drains the queue and moves what is left THEN.  -> [(level, count)].  (A model of the host loop for choosing seeds on the CPU: the trace
    of the GPU run is the authority.)"""
    max_steps = cap + 1
    counter = active_counts(iterations, max_steps)
    launched = checked = waited = nchunks = 0
    last, cur, level, moves, done = B, B, 0, [], False

    def enqueue():
        nonlocal launched, nchunks
        launched += min(CHECK_EVERY, max_steps - launched); nchunks += 1
    enqueue()
    while not done and waited < nchunks:
        if rp_min > 0 and last >= 1 and last <= at * cur and cur >= rp_min:
            while checked < launched:
                last = counter[checked]; checked += 1
                if last == 0:
                    done = True
                    break
            waited = nchunks
            if done:
                break
            moves.append((level, last)); level += 1; cur = last
            if launched < max_steps:
                enqueue()
            continue
        if launched < max_steps:
            enqueue()
        upto = min(launched, (waited + 1) * CHECK_EVERY)
        while checked < upto:
            last = counter[checked]; checked += 1
            if last == 0:
                done = True
                break
        waited += 1
    return moves
