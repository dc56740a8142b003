"""The host loop of a solve does what it did before its decisions moved into csrc/solve_loop.h.  tests/golden/solve_loop_parent.json holds the
TRAJOPT_SYNC_DEBUG=1 trace of three small solves (tests/solve_loop_cases.py: a draining iLQR batch that moves through the repacked working
sets, an ALTRO solve with the early polish armed, an iLQR solve in list mode), recorded with tools/solve_loop_parent.py on an MI355X from the
library of the commit before.  Every batch step — its number, the B and Bp it ran with, the working-set level and the active count it was
planned with — every move, the number of batch steps and the iterations and status of every trajectory must be equal, entry for entry."""
import json
from pathlib import Path

import pytest

import solve_loop_cases as P

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "solve_loop_parent.json"


@pytest.mark.parametrize("name", list(P.CASES))
def test_host_trace_equals_the_parents(name, hip, capfd, monkeypatch):
    want = json.loads(GOLDEN.read_text())["cases"][name]
    got = P.run(name, hip, monkeypatch.setenv, lambda: capfd.readouterr().err)
    assert P.is_real(name, want) and P.is_real(name, got)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w)
        for key in w:
            assert g[key] == w[key], f"{name} solve {k}: {key}"
