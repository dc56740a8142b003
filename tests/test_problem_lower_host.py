"""The host-only lowering behind the oldest entry points, everything that needs no GPU: csrc/desc_lower.h lower_problem (to_create),
lower_constraint_params (to_set_constraint_params_batch), cost_linear_delta / cost_linear_zero (to_set_cost_linear_batch, to_set_cost) and the
one plant-parameter rule (to_set_model_params_batch, the policy rollouts), compiled as a program of its own — tests/host_shim/
problem_lower_harness.cpp, also under AddressSanitizer + UndefinedBehaviorSanitizer; nothing is loaded into python.  The expected classes and
messages are literals here: they are what trajopt_hip.hip returned while these checks stood inline in it."""
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
CHANGED = "change the model's dimensions or attitude representation"


def _harness(tmp_path, flags=()):
    exe = tmp_path / "problem_lower_harness"
    keys = re.search(r"constexpr int N_MODEL_KEYS = (\d+);", (CSRC / "handle.h").read_text()).group(1)   # the harness walks the keys the library has
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-DN_MODEL_KEYS=" + keys, "-I", str(SHIM), "-I", str(CSRC), str(SHIM / "problem_lower_harness.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-3000:], r.stderr[-1500:])
    return r.stdout


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    return _harness(tmp_path_factory.mktemp("problem_lower"))


def test_lowering_harness_under_asan_ubsan(tmp_path):
    """The tables of lower_problem, lower_constraint_params bit for bit against the loop it replaced (B = 1, 3, 65), the linear-term
    differences, the plant rule over every key and entry, and every refusal with its output untouched — built with the sanitizers."""
    _harness(tmp_path, SAN)


def test_refusals_class_and_message(harness_out):
    cases = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"^case (\w+) code (-?\d+) msg (.*)$", harness_out, flags=re.M)}
    DIM, ARG, ASSERT, UNSUP, NULL = capi.TO_ERR_DIMENSION_MISMATCH, capi.TO_ERR_ARGUMENT, capi.TO_ERR_ASSERTION, capi.TO_ERR_UNSUPPORTED, capi.TO_ERR_NULL
    steps = "time(Z[end]) ≈ tf: time steps are inconsistent with the final time"
    hybrid = "hybrid double integrator: params[1] (time steps of the first model) must be an integer in 1 .. N-2"
    rows = "per-trajectory b of a LinearConstraint: the rows of A must be linearly independent"
    want = {
        # A. lower_problem, in the order of its checks
        "null_desc": (NULL, "null descriptor"),
        "abi": (ARG, "ABI version mismatch"),
        "opts": (ARG, "solver option out of range: tolerances must be >= 0"),
        "order_abi_before_opts": (ARG, "ABI version mismatch"),
        "unknown_model": (UNSUP, "unknown model"),
        "dims": (DIM, "Objective state/control dimensions don't match model."),
        "few_knots": (ASSERT, "length(models) == N-1 requires N >= 2"),
        "batch": (ARG, "batch must be positive"),
        "time_span": (ASSERT, "tf > t0"),
        "time_span_nan": (ASSERT, "tf > t0"),
        "integrator": (UNSUP, "unknown integrator"),
        "dt_sign": (ASSERT, "dt must be positive"),
        "dt_sum": (ASSERT, steps),
        "no_costs": (ARG, "objective needs at least one cost function"),
        "null_costs": (ARG, "objective needs at least one cost function"),
        "cost_kind": (UNSUP, "unknown cost kind"),
        "hybrid_steps": (ARG, hybrid),
        "hybrid_fraction": (ARG, hybrid),
        "step_models": (NULL, "TO_MODEL_VECTOR needs step_models[N-1]"),
        "cost_index": (DIM, "cost_index outside the cost list"),
        "one_cost": (ARG, "Objective(stage, terminal, N) needs two cost functions"),
        "order_knots_before_cost_index": (ASSERT, "length(models) == N-1 requires N >= 2"),
        "con_count": (ARG, "bad constraint list"),
        "con_null": (ARG, "bad constraint list"),
        "con_kind": (UNSUP, "unknown constraint kind"),
        "con_knots": (ASSERT, "Invalid inds, inds[end] must be less than number of knotpoints"),
        "fine_two_knots": (capi.TO_OK, ""),
        "fine_five_knots": (capi.TO_OK, ""),
        "dt_just_inside": (capi.TO_OK, ""),
        "dt_just_outside": (ASSERT, steps),
        "fine_constrained": (capi.TO_OK, ""),
        # B. lower_constraint_params (its two refusals exclude each other: the rank test is reached by a LinearConstraint only)
        "params_kind": (UNSUP, "per-trajectory constraint parameters: GoalConstraint (its target) and LinearConstraint (its b) only"),
        "params_equal_rows": (UNSUP, rows),
        "params_below_threshold": (UNSUP, rows),
        "params_above_threshold": (capi.TO_OK, ""),
        # C. cost_linear_delta
        "linear_both_null": (NULL, "null pointer"),
        "linear_error_quadratic": (UNSUP, "per-trajectory linear terms: not for ErrorQuadratic (its q slot carries x_ref)"),
        "order_null_before_kind": (NULL, "null pointer"),
        # D. validate_plant_params, as its two callers word it
        "plant_setter_not_finite": (ARG, "to_set_model_params_batch: entry 6 of trajectory 2 is not finite"),
        "order_not_finite_before_changed": (ARG, "to_set_model_params_batch: entry 6 of trajectory 2 is not finite"),
        "plant_setter_changed": (ARG, "to_set_model_params_batch: the parameters of trajectory 2 " + CHANGED),
        "plant_policy_changed": (ARG, "to_policy_rollout: plant_params " + CHANGED),
        "plant_policy_sample_changed": (ARG, "to_policy_rollout: plant_params of sample (b = 1, s = 2) " + CHANGED),
        "plant_model_vector": (ARG, "to_policy_rollout: a model vector takes no plant_params (its models live in the step table)"),
        "plant_policy_nan_passes": (capi.TO_OK, ""),
    }
    assert set(cases) == set(want)
    for k, (code, text) in want.items():
        assert cases[k] == (code, text), (k, cases[k])
    assert capi._ERRORS[ARG] is T.ArgumentError and capi._ERRORS[UNSUP] is T.UnsupportedError and capi._ERRORS[DIM] is T.DimensionMismatch


def test_minimum_norm_shift_meets_its_property(harness_out):
    """A shift[inds] = params_b - b0 for every trajectory, zero off inds: the harness allows the new code the residual of the loop it replaced on the
    same inputs (in effect equality) and reports the largest one seen.  That the replaced loop itself is a meaningful yardstick is held to
    1e-9 there and here: eps (2.2e-16) times the O(1) entries times a condition number of A A' below 1e6 for the seeded matrices."""
    m = re.search(r"^max_residual (\S+)$", harness_out, flags=re.M)
    assert m, harness_out[-500:]
    print("largest residual of A shift[inds] = params_b - b0:", m.group(1))
    assert float(m.group(1)) < 1e-9


def test_the_lowering_left_the_hip_translation_unit():
    src = (CSRC / "trajopt_hip.hip").read_text()
    assert "std::sqrt(" not in src and "check_plant_params" not in src
    hits = [f.name for f in sorted(CSRC.iterdir()) if f.suffix in (".h", ".hip") and CHANGED in f.read_text()]
    assert hits == ["desc_lower.h"]
    # the entry points call the lowering by name (to_create: no refusal of its own ahead of the device count)
    body = src[src.index("int to_create("):src.index("hipGetDeviceCount(&ndev)")]
    assert "lower_problem(" in body and "return fail(" not in body
    for name in ("lower_constraint_params(", "cost_linear_delta(", "cost_linear_zero(", "validate_plant_params("):
        assert name in src, name
