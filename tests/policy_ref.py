"""The closed-loop policy rollout restated on the CPU, shared by tests/test_gpu_policy_rollout.py (the HIP kernel on the MI355X) and
tests/test_policy_host.py (the same kernel text compiled for the host).

``restate`` steps with the oracle's ``discrete_dynamics`` and ``state_diff`` in the order the header gives and takes the nominal trajectory and
the gains from its caller, so only the rollout is under test.  J and c_max come from the oracle itself (``oracle_cost_and_violation``): a
sample's closed-loop (X, U) is loaded into an oracle problem and evaluated with T.cost / T.max_violation.

Tolerance RTOL = 1e-9 (relative, max norm per sample): open-loop rollouts are held to 1e-11 (test_gpu_parity.py::test_rollout_and_cost) and the
closed loop amplifies a 1e-9 relative disturbance of K at most 112-fold at these shapes, so rounding stays orders of magnitude below.
"""
import ctypes as C

import numpy as np

import trajopt_amd as T

PD = C.POINTER(C.c_double)
RTOL = 1e-9


class Stepper:
    """One time step / one state difference through the oracle, on buffers bound once (the restatement makes ~10^5 calls)."""

    def __init__(self, oracle, prob, plant=None):
        self.prob, model = prob, prob.model
        self.n, self.ne = prob.n, prob.errstate_dim
        self.x, self.x0, self.u, self.xn, self.dx = np.zeros(prob.n), np.zeros(prob.n), np.zeros(prob.m), np.zeros(prob.n), np.zeros(self.ne)
        self.px, self.px0, self.pu, self.pxn, self.pdx = (a.ctypes.data_as(PD) for a in (self.x, self.x0, self.u, self.xn, self.dx))
        self.step_fn, self.diff_fn = oracle.raw("discrete_dynamics"), oracle.raw("state_diff")
        self.hybrid = isinstance(model, T.HybridDoubleIntegrator)
        self.dt = np.diff(prob.gettimes())

        def params(mod):
            p = list((plant or mod).params()) + [0.0] * 16
            return (C.c_double * 16)(*p[:16])
        if self.hybrid:   # the oracle steps a model vector per knot only inside its own rollout: restate the three phases
            self.subs = [(mod, None if isinstance(mod, T.DiscreteMap) else params(mod)) for mod in model.models(prob.N)]
        else:
            self.params, self.model_id = params(model), model.model_id
        self.diff_params = (C.c_double * 16)(*(list(model.params()) + [0.0] * 16)[:16])

    def step(self, k, x, u):
        if self.hybrid:
            mod, par = self.subs[k]
            out = np.zeros(self.n)
            if par is None:                                    # the jump map (4, 2) -> 2
                out[0], out[1] = 0.5 * (x[2] + x[3]), 0.5 * (u[0] + u[1])
                return out
            self.x[:] = 0.0; self.u[:] = 0.0; self.xn[:] = 0.0
            self.x[:mod.n] = x[:mod.n]; self.u[:mod.m] = u[:mod.m]
            assert self.step_fn(mod.model_id, par, self.prob.integration, self.px, self.pu, float(self.dt[k]), self.pxn) == 0
            out[:mod.n] = self.xn[:mod.n]
            return out
        self.x[:] = x; self.u[:] = u
        assert self.step_fn(self.model_id, self.params, self.prob.integration, self.px, self.pu, float(self.dt[k]), self.pxn) == 0
        return self.xn.copy()

    def diff(self, x, x0):
        if self.hybrid:
            return x - x0
        self.x[:] = x; self.x0[:] = x0
        assert self.diff_fn(self.prob.model.model_id, self.diff_params, self.px, self.px0, self.pdx) == 0
        return self.dx.copy()


def restate(oracle, prob, Xbar, Ubar, K, d, X0s, alpha=0.0, u_min=None, u_max=None, plant=None):
    """The operator, restated: per sample x_1 = X0s[b, s]; for k = 1 .. N-1: dx = state_diff(x_k, x̄_k), u_k = ū_k + α d_k + K_k dx clamped,
    |dx| accumulated, x_{k+1} = plant step; then the terminal |dx|.  -> X [B,S,N,n], U [B,S,N-1,m], dx_max [B,S]."""
    B, S, N, n, m = prob.B, X0s.shape[1], prob.N, prob.n, prob.m
    st = Stepper(oracle, prob, plant)
    X, U, dxm = np.zeros((B, S, N, n)), np.zeros((B, S, N - 1, m)), np.zeros((B, S))
    for b in range(B):
        for s in range(S):
            x = X0s[b, s].copy()
            worst = 0.0
            for k in range(N - 1):
                X[b, s, k] = x
                dx = st.diff(x, Xbar[b, k])
                u = Ubar[b, k] + alpha * d[b, k] + K[b, k] @ dx
                if u_min is not None:
                    u = np.maximum(u, u_min)
                if u_max is not None:
                    u = np.minimum(u, u_max)
                U[b, s, k] = u
                worst = max(worst, np.abs(dx).max())
                x = st.step(k, x, u)
            X[b, s, N - 1] = x
            dxm[b, s] = max(worst, np.abs(st.diff(x, Xbar[b, N - 1])).max())
    return X, U, dxm


def oracle_cost_and_violation(oracle, build, X, U):
    """J and c_max of every closed-loop sample from the oracle: the samples loaded as the trajectories of one oracle problem,
    ``build(oracle, batch)``."""
    B, S = X.shape[:2]
    po = build(oracle, B * S)
    T.initial_states(po, X.reshape(B * S, *X.shape[2:]))
    T.initial_controls(po, U.reshape(B * S, *U.shape[2:]))
    return T.cost(po).reshape(B, S), T.max_violation(po).reshape(B, S)


def sample_starts(prob, Xbar, sigma, S, seed=11):
    rng = np.random.default_rng(seed)
    X0s = Xbar[:, None, 0, :] + sigma * rng.standard_normal((prob.B, S, prob.n))
    X0s[:, 0] = Xbar[:, 0]
    if isinstance(prob.model, T.Quadrotor) and prob.n == 13:
        X0s[..., 3:7] /= np.linalg.norm(X0s[..., 3:7], axis=-1, keepdims=True)
    return np.ascontiguousarray(X0s)


def compare(name, r, ref, rtol=RTOL):
    """X, U, dx_max, J at rtol relative in the max norm per sample; c_max at rtol + 1e-12; status all 0.  Prints the largest deviations."""
    Xr, Ur, dxr, Jr, cr = ref
    B, S = Jr.shape
    assert r.X.shape == Xr.shape and r.U.shape == Ur.shape and r.J.shape == (B, S)
    np.testing.assert_array_equal(r.status, 0)
    np.testing.assert_array_equal(r.k_limit, 0)

    def rel(a, b):
        a, b = a.reshape(B * S, -1), b.reshape(B * S, -1)
        return np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))
    dev = {"X": rel(r.X, Xr), "U": rel(r.U, Ur), "dx_max": rel(r.dx_max, dxr), "J": rel(r.J, Jr)}
    print(f"policy_rollout deviation {name}: " + " ".join(f"{k}={v.max():.2e}" for k, v in dev.items())
          + f" c_max={np.abs(r.c_max - cr).max():.2e}")
    for k, v in dev.items():
        bad = np.where(~(v <= rtol))[0]
        assert bad.size == 0, f"{name} {k}: samples {bad[:8]} off by {v[bad[:8]]} (allowed {rtol})"
    np.testing.assert_allclose(r.c_max, cr, rtol=rtol, atol=1e-12)


def ref_slice(ref, S):
    return tuple(a[:, :S] for a in ref)
