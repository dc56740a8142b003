"""Problem(models::Vector{<:DiscreteDynamics}, ...) in general (src/problem.jl:36-73, src/dynamics.jl:15-31): any mix
of the compiled-in step models — DoubleIntegrator (D = 1, 2, 3), Cartpole, LinearMap — whose dimensions chain, through the
per-step table TO_MODEL_VECTOR (stored at (6, 3), narrower knots zero-padded).  Pinned without a GPU: the oracle's solve of an
all-linear mix against a numpy Riccati recursion written at the TRUE per-knot dimensions (6,3) -> 4 -> (4,2) -> 2 -> (2,1); a mix
with the nonlinear Cartpole against per-segment rollouts and finite differences; the validation errors of RD.dims.  The GPU is
compared with the oracle in tests/test_gpu_parity.py::test_general_model_vector_on_gpu."""
import ctypes as C

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I


def linear_mix(mass=1.3):
    rng = np.random.default_rng(12)
    j1 = T.LinearMap(rng.uniform(-0.5, 0.5, (4, 6)) + np.eye(4, 6), rng.uniform(-0.3, 0.3, (4, 3)))      # (6, 3) -> 4
    j2 = T.LinearMap(np.array([[0, 0, .5, .5], [1.0, -1.0, 0, 0]]), np.array([[.5, .5], [0, 0.2]]))     # (4, 2) -> 2
    return [T.DoubleIntegrator(mass, 3)] * 3 + [j1] + [T.DoubleIntegrator(mass, 2)] * 3 + [j2] + [T.DoubleIntegrator(mass, 1)] * 3


def cartpole_mix():
    j = T.LinearMap(np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0]]), np.array([[0.0], [0.1]]))                # (4, 1) -> 2: cart position / velocity
    return [T.DoubleIntegrator(1.0, 2)] * 3 + [T.Cartpole()] * 6 + [j] + [T.DoubleIntegrator(2.0, 1)] * 3


def build(models, lib, batch=3, constrained=False, tf=None, seed=5, integration=T.RK4):
    nx, nu = T.dims(models)
    N = len(models) + 1
    rng = np.random.default_rng(seed)
    costs = [T.LQRCost(rng.uniform(0.5, 2.0, n), rng.uniform(0.05, 0.3, m), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.2, 0.2, m))
             for n, m in zip(nx, nu)]
    cons = T.ConstraintList(models)
    if constrained:
        T.add_constraint(cons, T.BoundConstraint(nx[0], nu[0], u_max=0.8, u_min=-0.8), range(1, 3))
        T.add_constraint(cons, T.GoalConstraint(np.array([0.3, -0.2])), N)
    x0 = rng.uniform(-0.4, 0.4, (batch, nx[0]))
    prob = T.Problem(models, T.Objective(costs), x0[0], tf or 0.1 * (N - 1), constraints=cons, batch=batch, lib=lib, integration=integration)
    prob.set_initial_state(np.c_[x0, np.zeros((batch, prob.n - nx[0]))])
    return prob, costs, x0


def step_maps(models, dt):
    maps = []
    for mod in models:
        if isinstance(mod, T.LinearMap):
            maps.append((mod.A, mod.B))
        else:  # RK4 of a double integrator is its exact Taylor series
            D, ms = mod.D, mod.mass
            A = np.eye(2 * D); A[:D, D:] = dt * np.eye(D)
            maps.append((A, np.vstack([dt * dt / (2 * ms) * np.eye(D), dt / ms * np.eye(D)])))
    return maps


def lqr_reference(maps, costs, x0):
    N = len(maps) + 1
    Q = [np.diag(c.Q) for c in costs]; R = [np.diag(c.R) for c in costs]; q = [c.q for c in costs]; r = [c.r for c in costs]
    S, s = Q[-1], q[-1]
    K, d = [None] * (N - 1), [None] * (N - 1)
    for k in range(N - 2, -1, -1):
        A, B = maps[k]
        Quu = R[k] + B.T @ S @ B; Qux = B.T @ S @ A; Qu = r[k] + B.T @ s
        K[k] = -np.linalg.solve(Quu, Qux); d[k] = -np.linalg.solve(Quu, Qu)
        Qxx = Q[k] + A.T @ S @ A; Qx = q[k] + A.T @ s
        S = Qxx + K[k].T @ Quu @ K[k] + K[k].T @ Qux + Qux.T @ K[k]
        s = Qx + K[k].T @ Quu @ d[k] + K[k].T @ Qu + Qux.T @ d[k]
    X, U, J = [np.asarray(x0, float)], [], 0.0
    for k in range(N - 1):
        u = K[k] @ X[k] + d[k]
        J += 0.5 * X[k] @ Q[k] @ X[k] + q[k] @ X[k] + 0.5 * u @ R[k] @ u + r[k] @ u + costs[k].c
        U.append(u); X.append(maps[k][0] @ X[k] + maps[k][1] @ u)
    J += 0.5 * X[-1] @ Q[-1] @ X[-1] + q[-1] @ X[-1] + costs[-1].c
    return X, U, J


def test_linear_mix_equals_per_knot_riccati(oracle):
    models = linear_mix()
    assert T.dims(models) == ([6] * 4 + [4] * 4 + [2] * 4, [3] * 4 + [2] * 4 + [1] * 4)
    prob, costs, x0 = build(models, oracle)
    assert isinstance(prob.model, T.ModelVector) and prob.hybrid and prob.knot_dims() == (prob.nx, prob.nu)
    sol = T.iLQRSolver(prob).solve()
    assert np.all(sol.stats["status"] == T.capi.SOLVE_SUCCEEDED)
    X, U = T.states(prob), T.controls(prob)
    maps = step_maps(models, prob.tf / (prob.N - 1))
    for b in range(prob.B):
        Xr, Ur, Jr = lqr_reference(maps, costs, x0[b])
        for k in range(prob.N):
            nk = prob.nx[k]
            np.testing.assert_allclose(X[b, k, :nk], Xr[k], rtol=1e-9, atol=1e-11, err_msg=f"knot {k + 1}")
            np.testing.assert_array_equal(X[b, k, nk:], 0.0)          # padding stays exactly zero
        for k in range(prob.N - 1):
            mk = prob.nu[k]
            np.testing.assert_allclose(U[b, k, :mk], Ur[k], rtol=1e-9, atol=1e-11, err_msg=f"step {k + 1}")
            np.testing.assert_array_equal(U[b, k, mk:], 0.0)
        assert sol.stats["cost"][b] == pytest.approx(Jr, rel=1e-11)
    I.expand(prob)
    A, B = I.dynamics_jacobians(prob)
    np.testing.assert_allclose(A[0, 3][:4, :6], models[3].A, rtol=0, atol=0)   # the (6, 3) -> 4 map, embedded in the padded blocks
    np.testing.assert_array_equal(A[0, 3][4:], 0.0)
    np.testing.assert_allclose(B[0, 7][:2, :2], models[7].B, rtol=0, atol=0)
    np.testing.assert_array_equal(B[0, 7][:, 2], 0.0)


def test_cartpole_mix_rollout_and_jacobians(oracle):
    models = cartpole_mix()
    prob, costs, x0 = build(models, oracle, batch=2)
    rng = np.random.default_rng(2)
    Uin = np.zeros((2, prob.N - 1, prob.m))
    for k, mk in enumerate(prob.nu[:-1]):
        Uin[:, k, :mk] = rng.uniform(-1, 1, (2, mk))
    T.initial_controls(prob, Uin)
    T.rollout(prob)
    X = T.states(prob)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    h = prob.tf / (prob.N - 1)

    def step(mod, x, u):                     # one time step of a stand-alone model at its own dimensions
        if isinstance(mod, T.LinearMap):
            return mod.A @ x + mod.B @ u
        xn = np.zeros(mod.n)
        params = (C.c_double * 16)(*(mod.params() + [0.0] * (16 - len(mod.params()))))
        oracle.call("discrete_dynamics", mod.model_id, params, T.RK4, pd(np.ascontiguousarray(x, dtype=np.float64)),
                    pd(np.ascontiguousarray(u, dtype=np.float64)), float(h), pd(xn))
        return xn

    for b in range(2):                       # per-segment rollout with the stand-alone models
        x = x0[b].copy()
        for k, mod in enumerate(models):
            x = step(mod, x, Uin[b, k, :mod.m])
            nk = prob.nx[k + 1]
            np.testing.assert_allclose(X[b, k + 1, :nk], x, rtol=1e-13, atol=1e-14, err_msg=f"knot {k + 2}")
            np.testing.assert_array_equal(X[b, k + 1, nk:], 0.0)
    # Jacobians of every padded step against central differences of the stand-alone step; zero outside the live block
    I.expand(prob)
    A, B = I.dynamics_jacobians(prob)
    e = 1e-6
    for k, mod in enumerate(models):
        x, u, no = X[0, k, :mod.n], Uin[0, k, :mod.m], prob.nx[k + 1]
        for j in range(mod.n):
            dx = np.zeros(mod.n); dx[j] = e
            np.testing.assert_allclose(A[0, k][:no, j], (step(mod, x + dx, u) - step(mod, x - dx, u)) / (2 * e), rtol=1e-6, atol=1e-8)
        for j in range(mod.m):
            du = np.zeros(mod.m); du[j] = e
            np.testing.assert_allclose(B[0, k][:no, j], (step(mod, x, u + du) - step(mod, x, u - du)) / (2 * e), rtol=1e-6, atol=1e-8)
        np.testing.assert_array_equal(A[0, k][no:], 0.0)
        np.testing.assert_array_equal(A[0, k][:, mod.n:], 0.0)
        np.testing.assert_array_equal(B[0, k][:, mod.m:], 0.0)


def test_cartpole_mix_constrained_solves(oracle):
    prob, costs, x0 = build(cartpole_mix(), oracle, constrained=True)
    s = T.ALTROSolver(prob).solve()
    assert np.all(s.stats["status"] == T.capi.SOLVE_SUCCEEDED) and s.stats["c_max"].max() <= 1e-6
    X, U = T.states(prob), T.controls(prob)
    np.testing.assert_allclose(X[:, -1, :2], [[0.3, -0.2]] * prob.B, atol=1e-6)
    assert np.all(np.abs(U[:, :2, :2]) <= 0.8 + 1e-6)
    np.testing.assert_array_equal(X[:, -1, 2:], 0.0)


def test_model_vector_validation(oracle):
    models = linear_mix()
    nx, nu = T.dims(models)
    bad = models[:3] + models[4:] + [models[-1]]                     # the first jump map removed: (6, 3) feeds a (4, 2) model
    with pytest.raises(T.DimensionMismatch, match=r"Model mismatch at time step 3\. Model 3 has an output dimension of 6 but model 4 has a state dimension of 4\."):
        T.dims(bad)
    with pytest.raises(T.DimensionMismatch):
        T.LinearMap(np.zeros((2, 4)), np.zeros((3, 1)))
    class Other(T.DoubleIntegrator):
        pass
    costs = [T.LQRCost(np.ones(n), np.ones(m), np.zeros(n)) for n, m in zip(nx, nu)]
    # the library checks the chain again on its side of the C-ABI (RD.dims' text): hand it a broken table directly
    prob, _, _ = build(models, oracle, batch=1)
    d = prob._desc
    steps = prob._steps
    steps[3].n_out = 5
    h = C.c_void_p()
    with pytest.raises(T.DimensionMismatch, match="Model mismatch at time step 4"):
        oracle.call("create", C.byref(d), None, 0, C.byref(h))
    steps[3].n_out = 4
    steps[0].kind = 7
    with pytest.raises(T.UnsupportedError):
        oracle.call("create", C.byref(d), None, 0, C.byref(h))
