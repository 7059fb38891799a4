#!/usr/bin/env python3
"""The record of tests/test_gpu_affective.py: the RoBERTa emotion classifier's and AffectiveForensics' measured error against their
float64 yardsticks, as the share of the bound each test holds it to (bf16 stages: 3 x the bf16-operand mirror's own error on the same
input, so a share of 1/3 is the mirror's own error; fp32-only stages: the rounding bounds of tests/affective_ref.py).  Runs the test
file in a child process on the MI355X and collects the figures every test prints before it asserts.

    python tools/affective_errors.py [--out profiles/affective_errors.txt] [--log FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_affective.py -m gpu -s` run on the MI355X instead of running one.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LINE = re.compile(r"AFFECTIVE_ERR (.+?) (\S+) err (\S+) bound (\S+)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.log:
        r = subprocess.CompletedProcess([], 0, stdout=Path(a.log).read_text(), stderr="")
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_affective.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"], cwd=str(REPO),
                           capture_output=True, text=True, timeout=900)
    rows = [m.groups() for m in LINE.finditer(r.stdout)]
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("affective_errors.py: the GPU tests printed no figures (no MI355X?)")
    worst, exact = {}, []
    for what, crit, err, bound in rows:
        kind, _, case = what.partition(" ")
        if kind == "exact":
            exact.append(f"{case} {crit}".replace(" bits equal", ": bits equal"))
            continue
        if kind == "stage":      # "stage <case> <name>": worst case per stage name
            case, _, stage = case.rpartition(" ")
            key = (kind, stage, crit)
        elif kind in ("embed", "arousal"):
            key = (kind, "", crit)
        else:
            key = (kind, case, crit)
        share = float(err) / float(bound) if float(bound) > 0 else 0.0
        if key not in worst or share > worst[key][0]:
            worst[key] = (share, case, float(err), float(bound))
    tail = r.stdout.strip().splitlines()[-1]
    lines = ["RoBERTa emotion classifier and AffectiveForensics on the MI355X against transformers.RobertaForSequenceClassification in float64,",
             "float64 restatements of the head and the arousal, and the real reference's recorded analyze() (tests/test_gpu_affective.py): worst",
             "case per stage and criterion, as err / bound.  bf16 stages (hidden*, logits, class_probs of `stage`): the bound is 3 x the",
             "bf16-operand mirror's own error on that input, so 0.33 is the mirror's error; everything else: fp32 rounding bounds.", ""]
    for (kind, stage, crit), (share, case, err, bound) in sorted(worst.items()):
        lines.append(f"  {kind:14s} {stage:22s} {crit:14s} {share:8.4f}   at {case or '-'} (err {err:.3e}, bound {bound:.3e})")
    lines += ["", "bit comparisons"] + ["  " + e for e in exact]
    lines += ["", f"pytest: {tail}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    if r.returncode != 0:
        raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
