#!/usr/bin/env python3
"""The record of tests/test_gpu_head_cases.py: the fusion head's and the NODE classifier's measured error against the float64
oracle, as a ratio to the float32 oracle's own error on the same input (the tests allow 3), with the worst ratio per check at the
top; and of tests/test_head_cases.py's mutants: how far each leaves the bounds, and what the older criteria (2e-5 / 5e-4) make
of it.  Runs both test files in child processes and collects the figures the tests print before they assert.

    python tools/head_errors.py [--out profiles/head_errors.txt] [--log FILE] [--cpu-log FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_head_cases.py -m gpu -s` run on the MI355X instead of
running one; --cpu-log FILE: the same for `pytest tests/test_head_cases.py -s -k mutant`.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
ERR = re.compile(r"HEAD_ERR (\S+) (\S+) gpu=(\S+) bound=(\S+) ratio_to_mirror=(\S+)")
TABLE = re.compile(r"HEAD_TABLE (\S+) cases=(\d+) gpu=(\S+) bound=(\S+) ratio_to_mirror=(\S+) at=(\S+)")
MUTANT = re.compile(r"HEAD_MUTANT (\S+) (\S+): worst error / bound (\S+) at (\S+); on the older criteria \(2e-5 / 5e-4\) (\S+) x tolerance")
MUTANT_AT = re.compile(r"HEAD_MUTANT_AT (\S+) (\S+) (\S+): error / bound (\S+)")
CHECKS = (("fwd", "fusion forward"), ("fbwd", "fusion backward alone"), ("cfwd", "classifier forward alone"),
          ("cbwd", "classifier backward alone"), ("chain", "chain with cross-entropy"))


def _run(args, log):
    if log:
        return subprocess.CompletedProcess([], 0, stdout=Path(log).read_text(), stderr="")
    return subprocess.run([sys.executable, "-m", "pytest", *args, "-s", "-q", "-p", "no:cacheprovider"], cwd=str(REPO), capture_output=True,
                          text=True, timeout=1800)


def _kind(name: str) -> str:
    return re.sub(r"trees\.\d+", "trees.*", name)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--cpu-log", default=None)
    a = ap.parse_args()
    r = _run(["tests/test_gpu_head_cases.py", "-m", "gpu"], a.log)
    rows = [m.groups() for m in ERR.finditer(r.stdout)]
    table = [m.groups() for m in TABLE.finditer(r.stdout)]
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("head_errors.py: the GPU tests printed no figures (no MI355X?)")
    cpu = _run(["tests/test_head_cases.py", "-k", "mutant"], a.cpu_log)
    mutants = [m.groups() for m in MUTANT.finditer(cpu.stdout)]
    per_check, per_kind = {}, {}
    for case, name, gpu, bound, ratio in rows:
        chk = name.split("/", 1)[0]
        rec = (float(ratio), case, name, float(gpu), float(bound))
        if chk not in per_check or rec[0] > per_check[chk][0]:
            per_check[chk] = rec
        k = _kind(name)
        n, worst = per_kind.get(k, (0, rec))
        per_kind[k] = (n + 1, max(worst, rec))
    for name, cases, gpu, bound, ratio, at in table:
        chk = name.split("/", 1)[0]
        rec = (float(ratio), "table of " + cases + ", worst at " + at, name, float(gpu), float(bound))
        if chk not in per_check or rec[0] > per_check[chk][0]:
            per_check[chk] = rec
    tail = r.stdout.strip().splitlines()[-1]
    lines = ["fusion head + NODE classifier on the MI355X against oracle/tier_a.py in float64 (tests/test_gpu_head_cases.py): GPU error /",
             "the float32 oracle's own error on the same input (its largest over 12 orders of summation, tests/head_cases.py).  The tests",
             "hold every vector of every case to 3.", "",
             "worst ratio per check"]
    for chk, title in CHECKS:
        if chk in per_check:
            ratio, case, name, gpu, bound = per_check[chk]
            lines.append(f"  {title:28s} {ratio:6.2f}   {name} at {case} (gpu {gpu:.3e}, bound {bound:.3e})")
    lines += ["", "the loss, judged over the table: max over the cases of the error relative to the loss, against 3 x the float32 oracle's same",
              "maximum"]
    for name, cases, gpu, bound, ratio, at in sorted(table):
        lines.append(f"  {name:34s} {float(ratio):6.2f}   {cases:>2s} cases, worst at {at} (gpu {float(gpu):.3e}, bound {float(bound):.3e})")
    lines += ["", "worst case per tensor (trees.* : all trees; (all): the pooled thresholds / tiny biases of a case), and how many comparisons"]
    for k, (n, (ratio, case, name, gpu, bound)) in sorted(per_kind.items()):
        lines.append(f"  {k:40s} {ratio:6.2f}   at {case} (gpu {gpu:.3e}, bound {bound:.3e}; {n} comparisons)")
    lines += ["", "mutants of the float32 oracle (tests/test_head_cases.py, CPU): worst error / bound (4 needed), and error / tolerance on the",
              "older criteria of the head tests (outputs 2e-5 max-abs, gradients 5e-4 of the tensor's scale; above 1 they fail there too)"]
    for mutant, case, w, at, old in mutants:
        lines.append(f"  {mutant:28s} {case:20s} {float(w):10.3g} x bound at {at:40s} older criteria {float(old):9.3g} x tolerance")
    lines += ["", "the same mutants at the row-sliced reductions' own gradients (thresholds, gates, leaf tables, tiny biases, evidence gates):",
              "error / bound (4 needed at each)"]
    for mutant, case, name, w in MUTANT_AT.findall(cpu.stdout):
        lines.append(f"  {mutant:28s} {case:20s} {float(w):10.3g} x bound at {name}")
    lines += ["", f"pytest: {tail}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    if r.returncode != 0 or cpu.returncode != 0:
        raise SystemExit(r.returncode or cpu.returncode)


if __name__ == "__main__":
    main()
