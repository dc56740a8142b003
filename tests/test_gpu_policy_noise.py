"""to_policy_rollout_mc on the MI355X: the policy rollout with process noise, measurement noise (both drawn in the kernel, csrc/noise.h)
and one plant per sample.

Expected values come from tests/policy_noise_ref.py: the numpy restatement of the generator, and ``restate_mc`` — the loop of
test_gpu_policy_rollout.restate with ``dx + v_k`` in the law and ``x_{k+1} = oracle_state_add(f(x_k, u_k), w_k)``, stepping with the oracle
on the nominal and the gains of the HIP handle, so only the new kernel instances are under test.  J and c_max come from the oracle on the
closed-loop (X, U), as in that file, whose cases, ``solved``, ``Stepper``, ``compare`` and tolerance are imported, not copied.

Tolerances.  Generator: 1e-13 absolute (|z| <= 8.7; log, sqrt, sin / cos at about 1 ulp each compose to a few 1e-15).  Rollouts: compare's
RTOL = 1e-9 — the noise values differ between device and numpy at the 1e-15 level and pass through the same closed loop whose
amplification that file bounds.  Everything that must not depend on WHERE a sample is computed (lane map, chunk, S, sample_offset,
traj_offset), and noise switched off, is held to equality.

Every parity comparison prints its largest deviation (``policy_rollout deviation ...``, visible with ``-s``).
OBSERVED on an MI355X: not recorded yet — this file has not run on a GPU.
"""
import ctypes as C

import numpy as np
import pytest

import trajopt_amd as T
from trajopt_amd import internal as I
from trajectoryoptimization_jl_amd import configs

import policy_noise_ref as R
from test_gpu_policy_rollout import CASES, Stepper, compare, oracle_cost_and_violation, ref_slice, solved, _quickstart

pytestmark = pytest.mark.gpu

S_VALUES = [1, 3, 64, 70]   # 1, 3: packed lane map; 64: one full uniform wave; 70: a second wave with 6 live lanes
SIGMA = {"cartpole5": 0.01, "cartpole70": 0.01, "quickstart": 0.01, "quadrotor": 0.002}
SEED = 2024
FIELDS = ("X", "U", "J", "c_max", "dx_max", "status", "k_limit")


def assert_same(a, b, msg="", fields=FIELDS):
    for k in fields:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{msg} {k}")


def noise_of(case, which="wv", **kw):
    sg = SIGMA[case]
    return T.PolicyNoise(SEED, sigma_w=sg if "w" in which else None, sigma_v=sg if "v" in which else None, **kw)


_refs = {}


def noisy_ref(case, which, S, hip, oracle, plants=None, tag=None):
    """Restatement of the first S samples of the case under noise kinds `which` (cached; S < 70 with both kinds shares the S = 70 one:
    a draw does not depend on S).  The noise must be visible: more than 1e-3 away from the noise-free reference in X."""
    c = solved(case, hip, oracle)
    if which == "wv" and plants is None and S < 70:
        return ref_slice(noisy_ref(case, which, 70, hip, oracle), S)
    key = (case, which, S, tag)
    if key not in _refs:
        nz = noise_of(case, which) if which else None
        Xr, Ur, dxr = R.restate_mc(oracle, c["p"], c["Xbar"], c["Ubar"], c["K"], c["d"], c["X0s"][:, :S], noise=nz, plants=plants, Stepper=Stepper)
        moved = np.abs(Xr - c["ref"][0][:, :S]).max()
        assert moved > 1e-3, f"{case} {which} {tag}: the reference moved by {moved:.1e} only: noise / plants silently off?"
        Jr, cr = oracle_cost_and_violation(oracle, case, Xr, Ur)
        _refs[key] = (Xr, Ur, dxr, Jr, cr)
    return _refs[key]


# ------------------------------------------------------------------------------------------------ 1. the generator on the device
@pytest.mark.parametrize("traj, sample, k, kind", [(0, 0, 0, 0), (4, 69, 29, 1), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 0), (70000, 123456, 200, 1)])
def test_generator_on_the_device(traj, sample, k, kind, hip):
    pairs = 70          # more than one pass of the wave over the pairs
    z = T.policy_noise_draws(hip, SEED, traj, sample, k, kind, pairs)
    z0, z1 = R.normal_pair(SEED, traj, sample, k, kind, np.arange(pairs))
    want = np.stack([z0, z1], axis=-1).ravel()
    dev = np.abs(z - want).max()
    print(f"policy noise: device vs numpy normals ({traj}, {sample}, {k}, {kind}): largest deviation {dev:.2e}")
    assert dev <= 1e-13
    with pytest.raises(T.ArgumentError, match="pairs"):
        T.policy_noise_draws(hip, SEED, traj, sample, k, kind, 257)
    with pytest.raises(T.ArgumentError, match="kind"):
        T.policy_noise_draws(hip, SEED, traj, sample, k, 2, 1)


# ------------------------------------------------------------------------------------------------ 2. parity with the restatement
@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("case", ["cartpole5", "quadrotor", "quickstart"])
def test_parity_with_the_restatement(case, S, hip, oracle):
    c = solved(case, hip, oracle)
    r = T.policy_rollout(c["p"], c["X0s"][:, :S], trajectories=True, noise=noise_of(case))
    compare(f"{case} w+v S={S}", r, noisy_ref(case, "wv", S, hip, oracle))
    s_only = T.policy_rollout(c["p"], c["X0s"][:, :S], noise=noise_of(case))     # the summary-only call gives the same numbers
    assert s_only.X is None and s_only.U is None
    assert_same(s_only, r, fields=FIELDS[2:])


@pytest.mark.parametrize("which, S", [("w", 3), ("v", 70)])
@pytest.mark.parametrize("case", ["cartpole5", "quadrotor", "quickstart"])
def test_parity_with_one_noise_kind(case, which, S, hip, oracle):
    c = solved(case, hip, oracle)
    r = T.policy_rollout(c["p"], c["X0s"][:, :S], trajectories=True, noise=noise_of(case, which))
    compare(f"{case} {which} only S={S}", r, noisy_ref(case, which, S, hip, oracle))


# ------------------------------------------------------------------------------------------------ 3. off means identical
@pytest.mark.parametrize("S", [3, 70])
@pytest.mark.parametrize("case", ["cartpole5", "quadrotor"])
def test_off_means_identical(case, S, hip, oracle):
    c = solved(case, hip, oracle)
    p, x0s = c["p"], np.ascontiguousarray(c["X0s"][:, :S])
    plain = T.policy_rollout(p, x0s, trajectories=True)
    assert_same(T.policy_rollout(p, x0s, trajectories=True, noise=None), plain, "noise=None")
    assert_same(T.policy_rollout(p, x0s, trajectories=True, noise=T.PolicyNoise(SEED)), plain, "every pointer NULL")
    # ... and a NULL to_policy_noise* at the C-ABI itself
    J, st = np.empty((p.B, S)), np.empty((p.B, S), np.int32)
    out, o = T.capi.PolicyResult(), T.capi.PolicyOpts()
    out.J, out.status, o.refresh_gains = p._pd(J), p._pi(st), 1
    p._call("policy_rollout_mc", S, p._pd(x0s), C.byref(o), None, C.byref(out))
    np.testing.assert_array_equal(J, plain.J)
    np.testing.assert_array_equal(st, plain.status)


# ------------------------------------------------------------------------------------------------ 4. counter-based, not position-based
@pytest.mark.parametrize("case", ["cartpole5", "quadrotor"])
def test_draws_do_not_depend_on_the_lane_map_or_the_chunk(case, hip, oracle, monkeypatch):
    c = solved(case, hip, oracle)
    p = c["p"]
    uniform = T.policy_rollout(p, c["X0s"][:, :64], trajectories=True, noise=noise_of(case))
    monkeypatch.setenv("TRAJOPT_POLICY_MAP", "packed")
    packed = T.policy_rollout(p, c["X0s"][:, :64], trajectories=True, noise=noise_of(case))
    monkeypatch.delenv("TRAJOPT_POLICY_MAP")
    assert_same(packed, uniform, f"{case} S=64 packed vs uniform")
    whole = T.policy_rollout(p, c["X0s"], trajectories=True, noise=noise_of(case))
    monkeypatch.setenv("TRAJOPT_POLICY_CHUNK_WAVES", "1")
    parts = T.policy_rollout(p, c["X0s"], trajectories=True, noise=noise_of(case))
    monkeypatch.delenv("TRAJOPT_POLICY_CHUNK_WAVES")
    assert_same(parts, whole, f"{case} S=70 one wave per chunk")


@pytest.mark.parametrize("case", ["cartpole5", "quadrotor"])
def test_draws_do_not_depend_on_how_the_samples_are_split(case, hip, oracle):
    c = solved(case, hip, oracle)
    p = c["p"]
    whole = T.policy_rollout(p, c["X0s"], trajectories=True, noise=noise_of(case))
    head = T.policy_rollout(p, c["X0s"][:, :3], trajectories=True, noise=noise_of(case))
    tail = T.policy_rollout(p, c["X0s"][:, 3:], trajectories=True, noise=noise_of(case, sample_offset=3))
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(head, k), getattr(whole, k)[:, :3], err_msg=f"{case} first 3 of 70: {k}")
        np.testing.assert_array_equal(getattr(tail, k), getattr(whole, k)[:, 3:], err_msg=f"{case} samples 3..69 with sample_offset: {k}")


def test_a_shard_draws_what_the_whole_batch_draws(hip, oracle):
    """A second handle that holds trajectories 2..4 of the Cartpole batch, called with traj_offset = 2, gives rows 2..4."""
    c = solved("cartpole5", hip, oracle)
    whole = T.policy_rollout(c["p"], c["X0s"], trajectories=True, noise=noise_of("cartpole5"))
    q = CASES["cartpole5"]["build"](hip, 3)
    T.initial_states(q, c["Xbar"][2:5]); T.initial_controls(q, c["Ubar"][2:5])
    for S in (70, 3):
        shard = T.policy_rollout(q, c["X0s"][2:5, :S], trajectories=True, noise=noise_of("cartpole5", traj_offset=2))
        for k in FIELDS:
            np.testing.assert_array_equal(getattr(shard, k), getattr(whole, k)[2:5, :S], err_msg=f"S={S} {k}")
    other = T.policy_rollout(q, c["X0s"][2:5], trajectories=True, noise=noise_of("cartpole5"))    # without the offset: other draws
    assert np.abs(other.X - whole.X[2:5]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 5. one plant per sample
def _pole_masses(p, S):
    nominal = p.model
    return [[T.Cartpole(mc=nominal.mc, mp=nominal.mp * (1 + 0.2 * s / S), l=nominal.l, g=nominal.g) for s in range(S)] for _ in range(p.B)]


def test_plants_filled_with_one_plant_equal_the_plant_call(hip, oracle):
    c = solved("cartpole5", hip, oracle)
    p, nominal = c["p"], c["p"].model
    plant = T.Cartpole(mc=nominal.mc, mp=1.2 * nominal.mp, l=nominal.l, g=nominal.g)
    for S in (3, 70):
        one = T.policy_rollout(p, c["X0s"][:, :S], plant=plant, trajectories=True)
        many = T.policy_rollout(p, c["X0s"][:, :S], plants=[[plant] * S] * p.B, trajectories=True)
        assert_same(many, one, f"S={S}")
        pp = np.zeros((p.B, S, 16)); pp[..., :4] = plant.params()
        assert_same(T.policy_rollout(p, c["X0s"][:, :S], plants=pp, trajectories=True), one, f"S={S} as an array")


@pytest.mark.parametrize("S", [3, 70])
def test_every_sample_on_its_own_plant(S, hip, oracle):
    c = solved("cartpole5", hip, oracle)
    p = c["p"]
    plants = _pole_masses(p, S)
    r = T.policy_rollout(p, c["X0s"][:, :S], plants=plants, trajectories=True)
    compare(f"cartpole plants S={S}", r, noisy_ref("cartpole5", "", S, hip, oracle, plants=plants, tag="plants"))


def test_plants_with_noise_on_top(hip, oracle):
    c = solved("cartpole5", hip, oracle)
    p, S = c["p"], 3
    plants = _pole_masses(p, S)
    r = T.policy_rollout(p, c["X0s"][:, :S], plants=plants, trajectories=True, noise=noise_of("cartpole5"))
    compare("cartpole plants + w+v S=3", r, noisy_ref("cartpole5", "wv", S, hip, oracle, plants=plants, tag="plants"))


# ------------------------------------------------------------------------------------------------ 6. under the guard
@pytest.mark.parametrize("case", ["cartpole70", "quadrotor"])
def test_noise_and_plants_under_the_guard(case, hip, oracle, monkeypatch):
    """TRAJOPT_GUARD=1: the per-sample plants sit between red zones like every other array of the handle and are re-sized as S grows;
    the zones stay intact (a broken one fails the call) and the numbers are the unguarded ones."""
    c = solved(case, hip, oracle)

    def plants(S):
        pp = np.zeros((c["p"].B, S, 16))
        par = c["p"].model.params()
        pp[..., :len(par)] = par
        pp[..., 1 if case == "cartpole70" else 0] *= 1 + 0.2 * np.arange(S) / S       # pole mass / vehicle mass
        return pp
    sizes = (3, 70, 64)
    want = {S: T.policy_rollout(c["p"], c["X0s"][:, :S], plants=plants(S), noise=noise_of(case), trajectories=True) for S in sizes}
    monkeypatch.setenv("TRAJOPT_GUARD", "1")
    p = CASES[case]["build"](hip, CASES[case]["B"])
    T.initial_states(p, c["Xbar"]); T.initial_controls(p, c["Ubar"])
    monkeypatch.setenv("TRAJOPT_POLICY_CHUNK_WAVES", "2")
    for S in sizes:
        r = T.policy_rollout(p, c["X0s"][:, :S], plants=plants(S), noise=noise_of(case), trajectories=True)
        assert_same(r, want[S], f"{case} guard S={S}")
        np.testing.assert_array_equal(r.status, 0)


# ------------------------------------------------------------------------------------------------ 7. handle hygiene
@pytest.mark.parametrize("case", ["cartpole5", "quickstart"])
def test_a_noisy_call_leaves_the_handle_alone(case, hip, oracle):
    c = solved(case, hip, oracle)
    p = c["p"]
    I.expand(p); I.backwardpass(p)
    before = (T.states(p), T.controls(p), [I.get_duals(p, i) for i in range(len(p.constraints))], I.gains(p))
    plants = np.zeros((p.B, 3, 16)); plants[..., :len(p.model.params())] = p.model.params()
    T.policy_rollout(p, c["X0s"][:, :3], noise=noise_of(case), plants=plants, refresh_gains=False, trajectories=True)
    T.policy_rollout(p, c["X0s"], noise=noise_of(case), refresh_gains=False)
    after = (T.states(p), T.controls(p), [I.get_duals(p, i) for i in range(len(p.constraints))], I.gains(p))
    np.testing.assert_array_equal(before[0], after[0]); np.testing.assert_array_equal(before[1], after[1])
    for (l0, m0), (l1, m1) in zip(before[2], after[2]):
        np.testing.assert_array_equal(l0, l1); np.testing.assert_array_equal(m0, m1)
    for k in ("K", "d", "dV", "rho"):
        np.testing.assert_array_equal(before[3][k], after[3][k], err_msg=k)


@pytest.mark.parametrize("kind", ["cartpole_ilqr", "quickstart_al"])
def test_a_solve_after_noisy_calls_equals_a_fresh_handle(kind, hip):
    def make():
        if kind == "cartpole_ilqr":
            p = configs.cartpole_problem(batch=70, N=31, tf=3.0, lib=hip)
            return p, T.iLQRSolver(p)
        p = _quickstart(hip, 5)
        return p, T.ALSolver(p)
    pf, sf = make()
    sf.solve()
    ph, sh = make()
    T.rollout(ph)
    rng = np.random.default_rng(3)
    for S in (2, 70):
        x0s = T.states(ph)[:, None, 0, :] + 0.05 * rng.standard_normal((ph.B, S, ph.n))
        plants = np.zeros((ph.B, S, 16)); plants[..., :len(ph.model.params())] = ph.model.params()
        T.policy_rollout(ph, x0s, alpha=1.0, trajectories=True, noise=T.PolicyNoise(S, sigma_w=0.01, sigma_v=0.01), plants=plants)
    sh.solve()
    for k in sf.stats:
        np.testing.assert_array_equal(sh.stats[k], sf.stats[k], err_msg=k)
    np.testing.assert_array_equal(T.states(ph), T.states(pf))
    np.testing.assert_array_equal(T.controls(ph), T.controls(pf))


# ------------------------------------------------------------------------------------------------ 8. errors
def test_errors(hip, oracle):
    c = solved("cartpole5", hip, oracle)
    p = c["p"]
    x0s = np.ascontiguousarray(c["X0s"][:, :2])
    for bad in (-0.1, np.nan, np.inf, [0.1, 0.1, -1e-300, 0.1]):
        for name in ("sigma_w", "sigma_v"):
            with pytest.raises(T.ArgumentError, match=name + " must be finite and >= 0"):
                T.policy_rollout(p, x0s, noise=T.PolicyNoise(1, **{name: bad}))
    # a sigma on the hybrid model: refused, with the reason; its per-sample plants are served
    h = CASES["hybrid"]["build"](hip, 3)
    T.rollout(h)
    xh = np.ascontiguousarray(T.states(h)[:, None, 0, :])
    for name in ("sigma_w", "sigma_v"):
        with pytest.raises(T.capi.UnsupportedError, match="padded coordinates"):
            T.policy_rollout(h, xh, noise=T.PolicyNoise(1, **{name: 0.01}))
    hp = np.zeros((3, 1, 16)); hp[..., :len(h.model.params())] = h.model.params()
    assert_same(T.policy_rollout(h, xh, plants=hp, trajectories=True), T.policy_rollout(h, xh, trajectories=True), "hybrid plants")
    # both plant sources (the Python wrapper refuses this itself: straight to the C-ABI)
    out, o, nz = T.capi.PolicyResult(), T.capi.PolicyOpts(), T.capi.PolicyNoise()
    pp, pps = np.zeros(16), np.zeros((p.B, 2, 16))
    pp[:4] = p.model.params(); pps[..., :4] = p.model.params()
    o.refresh_gains, o.plant_params, nz.plant_params = 1, p._pd(pp), p._pd(pps)
    with pytest.raises(T.ArgumentError, match="both"):
        p._call("policy_rollout_mc", 2, p._pd(x0s), C.byref(o), C.byref(nz), C.byref(out))
    # what to_policy_rollout refuses
    nz = T.capi.PolicyNoise()
    with pytest.raises(T.ArgumentError, match="S must be"):
        p._call("policy_rollout_mc", 0, p._pd(x0s), None, C.byref(nz), C.byref(out))
    with pytest.raises(ValueError, match="x0s is NULL"):
        p._call("policy_rollout_mc", 2, None, None, C.byref(nz), C.byref(out))
    with pytest.raises(ValueError, match="out is NULL"):
        p._call("policy_rollout_mc", 2, p._pd(x0s), None, C.byref(nz), None)
    p._call("policy_rollout_mc", 2, p._pd(x0s), None, C.byref(nz), C.byref(out))     # NULL options = the defaults; every output may be NULL
    # one sample whose plant has another attitude representation: the message names it
    q = configs.quadrotor_problem(batch=2, N=11, tf=0.5, lib=hip)
    T.rollout(q)
    xq = np.ascontiguousarray(np.repeat(T.states(q)[:, None, 0, :], 3, axis=1))
    qp = np.zeros((2, 3, 16)); qp[..., :11] = q.model.params()
    T.policy_rollout(q, xq, plants=qp)
    qp[1, 2, 10] = 1.0
    with pytest.raises(T.ArgumentError, match=r"sample \(b = 1, s = 2\).*attitude representation"):
        T.policy_rollout(q, xq, plants=qp)
    # while a solve is in flight the handle refuses the call like any other
    big = configs.quadrotor_problem(batch=256, N=101, tf=5.0, lib=hip)
    s = T.iLQRSolver(big)
    s.solve_async()
    try:
        with pytest.raises(T.ArgumentError, match="in flight"):
            T.policy_rollout(big, np.zeros((big.B, 1, big.n)), noise=T.PolicyNoise(1, sigma_w=0.01))
    finally:
        s.wait()
