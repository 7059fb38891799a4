"""The record of tests/focal_cases.py: the worst error / bound of the float32 restatement, the best error / bound of every mutant and the
restatement against the reference fixture (CPU), and -- with --gpu, on the MI355X -- the worst error / bound of ufnd_softmax_focal per
batch size and per (alpha, gamma), and the device against tests/golden/recipe.npz.

    python tools/focal_mixup_errors.py [--gpu] [--out profiles/focal_mixup_errors.txt]

Without --gpu the kernel lines are left out: nothing measured on a CPU is ever written under a GPU heading."""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests import focal_cases as F  # noqa: E402

OP = F.OPS["focal"]
NOTES = """notes on shares above 0.5 (why a correct kernel attains them)
  every output reaches ~0.92 on rows with a gap of 12 whose label names the winner, at every gamma: S = 1 + exp(-gap) is rounded at u S
  (one addition), and ce = log(S) ~ exp(-gap) carries that absolute error whole; the bound's d_S / S term is this one rounding (the
  same share as the cross-entropy entry's), and fl and its gradient are products with ce.  The float32 restatement attains the same
  0.917: the device adds nothing visible to it.
"""


def cpu_ratio(mutant=None):
    worst, where = 0.0, None
    for case in OP.cases:
        inp = OP.make(case)
        r = max(F.check(case, inp, OP.restate(case, inp, mutant)).values())
        if r > worst:
            worst, where = r, case
        if worst == math.inf or (mutant is not None and worst >= F.MUTANT_FACTOR):
            break
    return worst, where


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["error / bound of ufnd_softmax_focal (bounds: tests/focal_cases.py; zero_rows is an exact family: 0 = equal, inf = a row differs)", ""]
    if a.gpu:
        import torch
        from tests import test_gpu_focal_mixup as G
        from tests.helpers import load_npz
        prop = torch.cuda.get_device_properties(0)
        lines.append(f"kernel on the GPU ({prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs; worst over the cases of the group)")
        by = {}
        for case in OP.cases:
            inp = OP.make(case)
            for k, r in F.check(case, inp, G.run_case(case, inp)).items():
                for key in (("B", case[0]), ("alpha, gamma", case[1]), ("output", k), ("mixup", case[4] is not None)):
                    if r > by.get(key, (-1.0, None))[0]:
                        by[key] = (r, case)
        for key in sorted(by, key=str):
            lines.append(f"  {key[0]:14s} {str(key[1]):14s} {by[key][0]:10.3g}   at {F.case_id(by[key][1])}")
        z = load_npz("recipe.npz")
        lg, ya, yb, m = z["focal/logits"], z["focal/labels_a"], z["focal/labels_b"], z["focal/moderate"]
        lines += ["", "the device against tests/golden/recipe.npz (the reference's own FocalLoss / mixup_criterion), error / (device bound + reference error)"]
        for k, (alpha, gamma) in enumerate(z["focal/alpha_gamma"]):
            for mixed in (False, True):
                mix = F.mix_of(float(z["focal/lam"])) if mixed else None
                full = G.run_focal(lg, ya, yb if mixed else None, mix, float(alpha), float(gamma))
                mod = G.run_focal(lg[m], ya[m], yb[m] if mixed else None, mix, float(alpha), float(gamma))
                r = F.fixture_checks(z, k, full["loss_rows"], float(full["loss"][0]), mod["d_logits"], mixed)
                lines.append(f"  alpha {alpha:<5g} gamma {gamma:<4g} {'mixed' if mixed else 'plain':6s} rows {r['rows']:9.3g}  mean {r['mean']:9.3g}  d_logits {r['d']:9.3g}")
        lines.append("")
    r, case = cpu_ratio()
    lines += ["float32 restatement on the CPU (worst over the cases; must be <= 1)", f"  {'focal':26s} {r:10.3g}   at {F.case_id(case)}", "",
              f"mutants on the CPU (up to the first case that leaves the bound by the factor; must be >= {F.MUTANT_FACTOR:g})"]
    for mu in F.MUTANTS:
        r, case = cpu_ratio(mu)
        lines.append(f"  {mu:38s} {r:10.3g}   at {F.case_id(case)}")
    lines += ["", NOTES.rstrip()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
