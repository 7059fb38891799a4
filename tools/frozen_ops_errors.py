"""The record of tests/frozen_ops_cases.py: per op the worst error / bound of the float32 restatement and the best error / bound
of every mutant (CPU), and -- with --gpu, on the MI355X -- the worst error / bound of the kernel itself and the case it came from.

    python tools/frozen_ops_errors.py [--gpu] [--out profiles/frozen_ops_errors.txt]

Without --gpu the kernel lines are left out: nothing measured on a CPU is ever written under a GPU heading."""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests import frozen_ops_cases as F  # noqa: E402


def cpu_ratio(op, mutant=None):
    worst, where = 0.0, None
    for case in F.OPS[op].cases:
        inp = F.OPS[op].make(case)
        with np.errstate(invalid="ignore"):
            r = max(F.check(op, case, inp, F.OPS[op].restate(case, inp, mutant)).values())
        if r > worst:
            worst, where = r, case
        if worst == math.inf:
            break
    return worst, where


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["error / bound per op (bounds: tests/frozen_ops_cases.py; 0 = bit-equal where the bound is 0, inf = a bit differs there)", ""]
    if a.gpu:
        import torch
        from tests import test_gpu_frozen_ops as G
        prop = torch.cuda.get_device_properties(0)
        lines.append(f"kernel on the GPU ({prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs; worst over the op's cases)")
        for op in sorted(F.OPS):
            r, case, key = G.worst_of(op)
            lines.append(f"  {op:22s} {r:10.3g}   at {F.case_id(case)} ({key})")
        lines.append("")
    lines.append("float32 restatement on the CPU (worst over the op's cases; must be <= 1)")
    for op in sorted(F.OPS):
        r, case = cpu_ratio(op)
        lines.append(f"  {op:22s} {r:10.3g}   at {F.case_id(case) if case is not None else '-'}")
    lines += ["", f"mutants on the CPU (best over the op's cases, up to the first bit-unequal one; must be >= {F.MUTANT_FACTOR:g})"]
    for op in sorted(F.OPS):
        for m in F.OPS[op].mutants:
            r, case = cpu_ratio(op, m)
            lines.append(f"  {op:22s} {m:32s} {r:10.3g}   at {F.case_id(case)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
