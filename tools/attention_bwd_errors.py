"""The record of tests/attention_bwd_cases.py: per case the worst error / allowance and the number of elements outside
[RNE(ref - e), RNE(ref + e)] (exact cases: the number of unequal elements) of ctx, lse and dqkv -- of the float32 restatement (CPU)
and, with --gpu on the MI355X, of the kernels themselves; then what every mutant does to the first cases that catch it.

    python tools/attention_bwd_errors.py [--gpu] [--out profiles/attention_bwd_errors.txt]

Without --gpu the kernel lines are left out: nothing measured on a CPU is ever written under a GPU heading."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests import attention_bwd_cases as A  # noqa: E402


def _fmt(res) -> str:
    return "   ".join(f"{k} {r:8.3g} / {n:d}" for k, (r, n) in res.items())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["worst error / allowance and elements outside, per case (tests/attention_bwd_cases.py; exact cases: allowance = one value,",
             "0 = bit-equal, inf = a bit differs; rounded cases: must be <= 1 with 0 outside)", ""]
    inputs = [A.make(c) for c in A.CASES]
    refs = [A.reference(c, inp) for c, inp in zip(A.CASES, inputs)]
    if a.gpu:
        import torch
        from tests import test_gpu_attention_bwd as G
        prop = torch.cuda.get_device_properties(0)
        lines.append(f"kernels on the GPU ({prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)")
        worst = {"exact": {}, "rounded": {}}
        for i, c in enumerate(A.CASES):
            res = A.check(c, G.run_case(c, inputs[i]), refs[i])
            kind = "exact" if A.is_exact(c) else "rounded"
            lines.append(f"  {A.case_id(c):44s} {kind:8s} {_fmt(res)}")
            for k, (r, n) in res.items():
                w = worst[kind].setdefault(k, [0.0, 0])
                w[0], w[1] = max(w[0], r), w[1] + n
        for kind in ("exact", "rounded"):
            lines.append(f"  worst over the {kind} cases: " + "   ".join(f"{k} {w[0]:.3g} / {w[1]}" for k, w in worst[kind].items()))
        lines.append("")
    lines.append("float32 restatement on the CPU")
    for i, c in enumerate(A.CASES):
        res = A.check(c, A.restate(c, inputs[i]), refs[i])
        lines.append(f"  {A.case_id(c):44s} {'exact' if A.is_exact(c) else 'rounded':8s} {_fmt(res)}")
    lines += ["", f"mutants on the CPU (dqkv of the first three cases that catch each, and for a mutant of the walk the first exact case with "
                    f"several walked blocks: a broken bit-equality or >= {A.MUTANT_FACTOR:g} x the allowance)"]
    for m in A.MUTANTS:
        hits, several = [], m not in A.WALK_MUTANTS       # a walk mutant: also the first exact case whose walk has several blocks
        for i, c in enumerate(A.CASES):
            if not A.mutant_applies(m, c) or c.L > 520:
                continue
            wanted = not several and A.is_exact(c) and c.L > A.WB
            if len(hits) >= 3 and not wanted:
                continue
            with np.errstate(invalid="ignore"):
                res = A.check(c, A.restate(c, inputs[i], m), refs[i])
            if A.caught(c, res):
                hits.append(f"{A.case_id(c)} {res['dqkv'][0]:.3g} / {res['dqkv'][1]}")
                several = several or wanted
            if len(hits) >= 3 and several:
                break
        lines.append(f"  {m:36s} " + ";  ".join(hits))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
