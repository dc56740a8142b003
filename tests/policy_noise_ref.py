"""numpy restatement of csrc/noise.h — Philox4x32-10, the two uniforms of a call, the Box-Muller pair — and of the stochastic policy
rollout (to_policy_rollout_mc) on top of the deterministic restatement of tests/test_gpu_policy_rollout.py.  Shared by
tests/test_policy_noise_host.py (against the C++ text compiled for the host) and tests/test_gpu_policy_noise.py (against the device)."""
import ctypes as C

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four broadcastable integer arrays (32-bit values), key: two integers -> four uint64 arrays holding the 32-bit output words."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*ctr)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]       # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniform_pair(seed, traj, sample, k, kind, j):
    seed = int(seed)
    r = philox4x32_10((traj, sample, k, np.asarray(kind, dtype=np.uint64) * np.uint64(256) + np.asarray(j, dtype=np.uint64)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    u1 = (((r[1] << np.uint64(32) | r[0]) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = (((r[3] << np.uint64(32) | r[2]) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return u1, u2


def normal_pair(seed, traj, sample, k, kind, j):
    u1, u2 = uniform_pair(seed, traj, sample, k, kind, j)
    r, a = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    return r * np.cos(a), r * np.sin(a)


def draws(seed, traj, sample, k, kind, ne):
    """z[..., ne]: the normals coordinate 0 .. ne-1 takes (pair j gives coordinates 2j and 2j+1; an odd ne discards the last normal).
    traj, sample, k broadcast against each other."""
    traj, sample, k = np.broadcast_arrays(np.asarray(traj), np.asarray(sample), np.asarray(k))
    j = np.arange((ne + 1) // 2)
    z0, z1 = normal_pair(seed, traj[..., None], sample[..., None], k[..., None], kind, j)
    return np.stack([z0, z1], axis=-1).reshape(*traj.shape, -1)[..., :ne]


def restate_mc(oracle, prob, Xbar, Ubar, K, d, X0s, noise=None, plants=None, alpha=0.0, Stepper=None):
    """to_policy_rollout_mc, restated: the loop of test_gpu_policy_rollout.restate with dx + v_k in the law, x_{k+1} = state_add(f(x_k, u_k),
    w_k) and the plant of sample (b, s) = plants[b][s] (models).  noise: a T.PolicyNoise.  -> X [B,S,N,n], U [B,S,N-1,m], dx_max [B,S]."""
    B, S, N, n, m, ne = prob.B, X0s.shape[1], prob.N, prob.n, prob.m, prob.errstate_dim
    zw = zv = None
    if noise is not None:
        bb, ss, kk = np.meshgrid(noise.traj_offset + np.arange(B), noise.sample_offset + np.arange(S), np.arange(N - 1), indexing="ij")
        if noise.sigma_w is not None:
            zw = np.broadcast_to(np.asarray(noise.sigma_w, dtype=float), (ne,)) * draws(noise.seed, bb, ss, kk, 0, ne)
        if noise.sigma_v is not None:
            zv = np.broadcast_to(np.asarray(noise.sigma_v, dtype=float), (ne,)) * draws(noise.seed, bb, ss, kk, 1, ne)
    shared = Stepper(oracle, prob) if plants is None else None
    add_fn = oracle.raw("state_add")
    PD = C.POINTER(C.c_double)
    xo, wbuf, xin = np.zeros(n), np.zeros(ne), np.zeros(n)
    par = (C.c_double * 16)(*(list(prob.model.params()) + [0.0] * 16)[:16])
    X, U, dxm = np.zeros((B, S, N, n)), np.zeros((B, S, N - 1, m)), np.zeros((B, S))
    for b in range(B):
        for s in range(S):
            st = shared if shared is not None else Stepper(oracle, prob, plants[b][s])
            x = X0s[b, s].copy()
            worst = 0.0
            for k in range(N - 1):
                X[b, s, k] = x
                dx = st.diff(x, Xbar[b, k])
                worst = max(worst, np.abs(dx).max())
                seen = dx if zv is None else dx + zv[b, s, k]
                u = Ubar[b, k] + alpha * d[b, k] + K[b, k] @ seen
                U[b, s, k] = u
                x = st.step(k, x, u)
                if zw is not None:
                    xin[:], wbuf[:] = x, zw[b, s, k]
                    assert add_fn(prob.model.model_id, par, xin.ctypes.data_as(PD), wbuf.ctypes.data_as(PD), xo.ctypes.data_as(PD)) == 0
                    x = xo.copy()
            X[b, s, N - 1] = x
            dxm[b, s] = max(worst, np.abs(st.diff(x, Xbar[b, N - 1])).max())
    return X, U, dxm
