#!/usr/bin/env python3
"""The record of tests/test_gpu_forgery.py: the measured error of the image-forgery evidence's float quantities (the gradient mean and std,
the score, the normalised vectors) against the mirror's float64 evaluation, as the share of the bound each test holds it to
(tests/forgery_ref.py: bounds of the reference's own float32 arithmetic), and the counts the tests print for the quantities held to
equality or one ulp.  Runs the test file in a child process on the MI355X and collects the figures every test prints before it asserts.

    python tools/forgery_errors.py [--out profiles/forgery_errors.txt] [--log FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_forgery.py -m gpu -s` run on the MI355X instead of running one.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LINE = re.compile(r"FORGERY_ERR (\S+) (\S+) err (\S+) bound (\S+)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.log:
        r = subprocess.CompletedProcess([], 0, stdout=Path(a.log).read_text(), stderr="")
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_forgery.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"], cwd=str(REPO),
                           capture_output=True, text=True, timeout=600)
    rows = [m.groups() for m in LINE.finditer(r.stdout)]
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("forgery_errors.py: the GPU tests printed no figures (no MI355X?)")
    worst, count = {}, {}
    for case, crit, err, bound in rows:
        crit = "vector (any dim)" if re.fullmatch(r"vec\d+", crit) else crit
        count[crit] = count.get(crit, 0) + 1
        err, bound = float(err), float(bound)
        share = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if crit not in worst or share > worst[crit][0]:
            worst[crit] = (share, case, err, bound)
    exact = [ln.strip().lstrip(".") for ln in r.stdout.splitlines() if "not bit-equal" in ln]
    tail = r.stdout.strip().splitlines()[-1]
    lines = ["Image-forgery evidence on the MI355X (tests/test_gpu_forgery.py): the gradient statistics, the score and the normalised vectors against the",
             "mirror's float64 evaluation.  Worst case per quantity over every image of the run, as err / bound; the bounds are those of the reference's",
             "float32 NumPy arithmetic (tests/forgery_ref.py), the device evaluates in double and rounds once.  A bound of 0 with err 0 marks a flat image",
             "(no gradient).  *_vs_reference rows compare with the numbers recorded from the reference itself, at twice the bound.  The resized and the",
             "round-tripped RGB, the ELA map, its luma, the histogram, max, min and mean are compared bit for bit by the tests and have no row here.", ""]
    for crit, (share, case, err, bound) in sorted(worst.items()):
        lines.append(f"  {crit:22s} {share:9.5f}   at {case} (err {err:.3e}, bound {bound:.3e}; {count[crit]} figures)")
    lines += ["", "counts"] + ["  " + e for e in exact]
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
