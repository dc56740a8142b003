#!/usr/bin/env python3
"""Instruction mix of one loop of a kernel, basic block by basic block (the static half of profiles/fwd2_roller_issue.md).
Compiles one translation unit to gfx950 assembly with the build's flags (as tools/spill_lanes_in_loops.py does, whose loop list
gives the line range), splits the range at labels and branches, and classifies every instruction: FP64 arithmetic, other VALU
(moves, v_cndmask, integer, compares), SALU, LDS, vector memory, waits and barrier, branches.  A block that the branch ending the
block before it jumps over is marked `skippable`: it runs only when that branch falls through (the trig slow paths of the rollout).
  python tools/loop_instruction_mix.py ops_small_forward2.hip _ZN2to10k_forward2INS_13CartpoleModelELi5E 1873 2360 [kept.s]
(a sixth argument names an assembly file kept from an earlier compile, e.g. of the parent commit, instead of compiling)"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import trajopt_amd  # noqa: E402,F401
from trajectoryoptimization_jl_amd import build as B  # noqa: E402

CLASSES = ("fp64", "valu", "salu", "lds", "vmem", "wait", "branch")


def classify(ins):
    op = ins.split()[0]
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op in ("s_waitcnt", "s_barrier", "s_nop"):
        return "wait"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "vmem"
    if op.startswith("v_"):
        arith = re.match(r"v_(fma|fmac|mul|add|rcp|rndne|max|min|ldexp|frexp_mant|trunc|fract|floor|ceil|div_\w+|rsq|sqrt)_f64", op)
        return "fp64" if arith else "valu"
    return "salu"


def main():
    tu, prefix, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    if len(sys.argv) > 5:
        txt = Path(sys.argv[5]).read_text().split("\n")
    else:
        with tempfile.TemporaryDirectory() as d:
            out = Path(d) / "k.s"
            subprocess.run([B.hipcc_path(), *B.flags_for(tu), "-S", "--cuda-device-only", "-o", str(out), str(B.CSRC / tu)], check=True, capture_output=True)
            txt = out.read_text().split("\n")
    start = next(i for i, l in enumerate(txt) if l.startswith(prefix))
    seg = txt[start + lo:start + hi + 1]
    blocks, cur = [], {"label": f"(line {lo})", "ins": [], "skippable": False}
    for line in seg:
        s = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m or s.startswith("; %bb."):
            if cur["ins"]:
                blocks.append(cur)
            cur = {"label": m.group(1) if m else s.split(":")[0][2:], "ins": [], "skippable": False}
            continue
        if re.match(r"(v_|s_|ds_|global_|buffer_|scratch_|flat_)", s):
            cur["ins"].append(s)
    if cur["ins"]:
        blocks.append(cur)
    for i in range(1, len(blocks) - 1):  # the block before ends in a conditional branch to the label of the block after
        last = blocks[i - 1]["ins"][-1].split()
        if last[0].startswith("s_cbranch") and last[1] == blocks[i + 1]["label"]:
            blocks[i]["skippable"] = True
    print(f"{prefix}, lines {lo}..{hi}\n\n| block | " + " | ".join(CLASSES) + " | all | |\n|---|" + "---|" * (len(CLASSES) + 2))
    tot = {True: dict.fromkeys(CLASSES, 0), False: dict.fromkeys(CLASSES, 0)}
    for b in blocks:
        c = dict.fromkeys(CLASSES, 0)
        for ins in b["ins"]:
            c[classify(ins)] += 1
            tot[b["skippable"]][classify(ins)] += 1
        print(f"| `{b['label']}` | " + " | ".join(str(c[k]) for k in CLASSES) + f" | {len(b['ins'])} | {'skippable' if b['skippable'] else ''} |")
    for sk, name in ((False, "every pass"), (True, "skippable")):
        print(f"| **{name}** | " + " | ".join(str(tot[sk][k]) for k in CLASSES) + f" | {sum(tot[sk].values())} | |")


if __name__ == "__main__":
    main()
