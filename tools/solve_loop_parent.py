#!/usr/bin/env python3
"""Records tests/golden/solve_loop_parent.json: the host trace (TRAJOPT_SYNC_DEBUG=1) of the solves of tests/solve_loop_cases.py — the fixture
of tests/test_gpu_solve_loop.py.  Run it on an MI355X against the library of the commit to pin (TRAJOPT_HIP_LIBRARY=<that build's
libtrajopt_hip.so>).  The trace is written by the C library: stderr is captured at file-descriptor level.

Usage: tools/solve_loop_parent.py [out.json]"""
import json
import os
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import trajopt_amd as T  # noqa: E402
import solve_loop_cases as P  # noqa: E402


class Stderr:
    """File descriptor 2 redirected into a temporary file; take() -> what was written since the last call."""

    def __enter__(self):
        self.file = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        sys.stderr.flush()
        os.dup2(self.file.fileno(), 2)
        self.pos = 0
        return self

    def take(self):
        sys.stderr.flush()
        self.file.seek(self.pos)
        data = self.file.read()
        self.pos += len(data)
        return data.decode(errors="replace")

    def __exit__(self, *exc):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        rest = self.take()
        self.file.close()
        if exc[0] is not None:
            sys.stderr.write(rest[-4000:])


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "solve_loop_parent.json"
    lib = T.load_hip_library()
    data = {"build_id": lib.build_id(), "cases": {}}
    for name in P.CASES:
        before = dict(os.environ)
        with Stderr() as err:
            solves = P.run(name, lib, os.environ.__setitem__, err.take)
        os.environ.clear()
        os.environ.update(before)
        for k, s in enumerate(solves):
            print(f"{name} solve {k}: {s['batch_steps']} batch steps, {len(s['steps'])} traced, moves {s['moves']}, iterations {sum(s['iterations'])}, "
                  f"statuses { {v: s['status'].count(v) for v in sorted(set(s['status']))} }")
        assert P.is_real(name, solves), name
        data["cases"][name] = solves
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(data, separators=(",", ":")) + "\n")
    print(f"wrote {out} ({out.stat().st_size} bytes) from build {lib.build_id()}")


if __name__ == "__main__":
    main()
