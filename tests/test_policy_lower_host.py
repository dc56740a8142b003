"""The host-only lowering of the closed-loop rollouts and the receding-horizon step, everything that needs no GPU: csrc/policy_lower.h
lower_policy_opts (what to_policy_rollout, to_policy_rollout_mc and to_mpc_advance run before their first device call) and lower_mpc_opts,
compiled as a program of its own — tests/host_shim/policy_lower_harness.cpp, also under AddressSanitizer + UndefinedBehaviorSanitizer;
nothing is loaded into python.  The expected classes and messages are literals here: they are what trajopt_hip.hip returned while these
checks stood inline in policy_prepare and to_mpc_advance."""
import re
import subprocess
from pathlib import Path

import pytest

import trajopt_amd as T
from trajopt_amd import capi

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "trajectoryoptimization.jl_amd" / "csrc"
SHIM = ROOT / "tests" / "host_shim"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _harness(tmp_path, flags=()):
    exe = tmp_path / "policy_lower_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "policy_lower_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-3000:], r.stderr[-1500:])
    return r.stdout


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    return _harness(tmp_path_factory.mktemp("policy_lower"))


def test_lowering_harness_under_asan_ubsan(tmp_path):
    """The kernel's NZ, the per-sample plants of a handle with its own (and with per-trajectory time steps), the clamp, the lane map under
    force_packed, the wave limit at the smallest batch that crosses it, MpcArgs::u_fill, and every refusal with its output untouched — built
    with the sanitizers."""
    _harness(tmp_path, SAN)


def test_refusals_class_and_message(harness_out):
    cases = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"^case (\w+) code (-?\d+) msg (.*)$", harness_out, flags=re.M)}
    ARG, UNSUP, NULL = capi.TO_ERR_ARGUMENT, capi.TO_ERR_UNSUPPORTED, capi.TO_ERR_NULL
    changed = "change the model's dimensions or attitude representation"
    sigma = ("to_policy_rollout_mc: sigma_w / sigma_v on a hybrid model or a model vector (their padded coordinates must stay exactly 0 and their live "
             "dimensions change per knot)")
    no_shift = "to_mpc_advance: not available for the NamedModel (TO_MODEL_HYBRID_DOUBLE_INTEGRATOR, TO_MODEL_VECTOR and TO_MODEL_INFEASIBLE cannot shift their plan)"
    want = {
        # lower_policy_opts, in the order of its checks
        "samples": (ARG, "to_policy_rollout: S must be >= 1"),
        "not_compiled": (UNSUP, "policy rollout not compiled for this model"),
        "refresh_gains": (ARG, "to_policy_rollout: refresh_gains must be 0 or 1"),
        "alpha": (ARG, "to_policy_rollout: alpha must be finite"),
        "plant": (ARG, "to_policy_rollout: plant_params " + changed),
        "plant_model_vector": (ARG, "to_policy_rollout: a model vector takes no plant_params (its models live in the step table)"),
        "sigma_hybrid": (UNSUP, sigma),
        "sigma_model_vector": (UNSUP, sigma),
        "sigma_w": (ARG, "to_policy_rollout_mc: sigma_w must be finite and >= 0"),
        "sigma_v": (ARG, "to_policy_rollout_mc: sigma_v must be finite and >= 0"),
        "both_plants": (ARG, "to_policy_rollout_mc: plant_params given both in the options (one plant) and in the noise (one per sample)"),
        "order_first_bad_sample": (ARG, "to_policy_rollout: plant_params of sample (b = 1, s = 2) " + changed),
        "mc_not_compiled": (UNSUP, "to_policy_rollout_mc: not compiled for this model"),
        "mc_not_in_mask": (UNSUP, "to_policy_rollout_mc: not compiled for this model"),
        "mc_own_plants_not_in_mask": (UNSUP, "to_policy_rollout_mc: not compiled for this model"),
        "too_large_uniform": (ARG, "to_policy_rollout: S * B is too large for one call"),
        "largest_uniform": (capi.TO_OK, ""),
        "too_large_packed": (ARG, "to_policy_rollout: S * B is too large for one call"),
        "largest_packed": (capi.TO_OK, ""),
        "clamp": (ARG, "to_policy_rollout: u_min must not exceed u_max"),
        "clamp_nan": (ARG, "to_policy_rollout: u_min must not exceed u_max"),
        "order_alpha_before_clamp": (ARG, "to_policy_rollout: alpha must be finite"),
        "order_samples_before_refresh": (ARG, "to_policy_rollout: S must be >= 1"),
        # lower_mpc_opts, in the order of its checks
        "mpc_null": (NULL, "to_mpc_advance: mpc is NULL"),
        "mpc_model_7": (UNSUP, no_shift),
        "mpc_model_8": (UNSUP, no_shift),
        "mpc_model_11": (UNSUP, no_shift),
        "mpc_shift_low": (ARG, "to_mpc_advance: shift must be in 1 .. N-2 = 9; got 0"),
        "mpc_shift_high": (ARG, "to_mpc_advance: shift must be in 1 .. N-2 = 9; got 10"),
        "mpc_guess": (ARG, "to_mpc_advance: guess must be TO_MPC_GUESS_CLOSED_LOOP (0) or TO_MPC_GUESS_NOMINAL (1)"),
        "mpc_tail": (ARG, "to_mpc_advance: tail must be TO_MPC_TAIL_HOLD (0) or TO_MPC_TAIL_FILL (1)"),
        "mpc_reserved": (ARG, "to_mpc_advance: reserved must be 0"),
        "mpc_fill_null": (NULL, "to_mpc_advance: TO_MPC_TAIL_FILL needs u_fill"),
        "mpc_fill_not_finite": (ARG, "to_mpc_advance: u_fill must be finite"),
        "order_model_before_shift": (UNSUP, no_shift),
        "order_shift_before_guess": (ARG, "to_mpc_advance: shift must be in 1 .. N-2 = 9; got 99"),
        "order_reserved_before_fill": (ARG, "to_mpc_advance: reserved must be 0"),
        "mpc_fill": (capi.TO_OK, ""),
        "mpc_fill_reads_m_entries": (capi.TO_OK, ""),
        "mpc_hold": (capi.TO_OK, ""),
    }
    assert set(cases) == set(want)
    for k, (code, text) in want.items():
        assert cases[k] == (code, text), (k, cases[k])
    assert capi._ERRORS[ARG] is T.ArgumentError and capi._ERRORS[UNSUP] is T.UnsupportedError


def test_the_entry_points_call_the_lowering():
    src = (CSRC / "trajopt_hip.hip").read_text()
    prepare = src[src.index("static int policy_prepare("):src.index("static int policy_staging(")]
    assert prepare.index("lower_policy_opts(") < prepare.index("use_device(h)") and "return fail(" not in prepare
    advance = src[src.index("int to_mpc_advance("):src.index("int to_mpc_shift_duals(")]
    assert advance.index("CHECK_IDLE(h)") < advance.index("lower_mpc_opts(") < advance.index("policy_prepare(") and "return fail(" not in advance
    assert "isfinite" not in src                                           # plants, sigmas, u_fill: all checked in the headers
    header = re.sub(r"//.*", "", (CSRC / "policy_lower.h").read_text())
    assert "to_handle" not in header and not re.search(r"\bhip[A-Z]", header)   # host-only: no handle, no HIP call
