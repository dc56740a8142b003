"""Handles that never call to_set_cost_weights_batch compute the bits they computed before the entry point existed.
tests/golden/cw_parent_bits.npz holds five small solves that run the GENERAL kernel variants — the ones a handle with weights is routed to
(tests/cw_parent_cases.py: per-trajectory goals, per-trajectory limits, a non-selector constraint, per-trajectory plants on the Cartpole at
N = 41, B = 70, and per-trajectory goals on the Quadrotor at B = 24) — recorded with tools/cw_parent_bits.py on an MI355X from the library
of the commit before per-trajectory cost weights were added.  Every stat of every trajectory and the kept trajectories' X / U must be
identical: the weights are a compile-time property of the kernel instances outside the forward pass (problem_dev.h cost_weights) and a
wave-uniform select inside it, where -ffp-contract=on forms the same fused operations either way."""
from pathlib import Path

import numpy as np
import pytest

import trajopt_amd as T
import cw_parent_cases as P

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "cw_parent_bits.npz"


@pytest.mark.parametrize("name", list(P.CASES))
def test_general_variants_without_weights_keep_their_bits(name, hip):
    g = np.load(GOLDEN)
    out = P.run(name, hip)
    assert (out[f"{name}_status"] == T.capi.SOLVE_SUCCEEDED).mean() > 0.9     # the recorded solves are real ones
    for k, v in out.items():
        np.testing.assert_array_equal(v, g[k], err_msg=k)
