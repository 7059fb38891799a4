#!/usr/bin/env python3
"""The record of tests/test_gpu_motion.py: the measured error of the video motion forensics' float statistics (ChronosGuard's seven,
the pyramid chunks' mean and std of m, the normalised vectors, cache_visual) against the mirror's float64 evaluation, as the share of
the bound each test holds it to (tests/motion_ref.py: bounds of the reference's own float32 arithmetic).  Runs the test file in a child
process on the MI355X and collects the figures every test prints before it asserts.

    python tools/motion_errors.py [--out profiles/motion_errors.txt] [--log FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_motion.py -m gpu -s` run on the MI355X instead of running one.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LINE = re.compile(r"MOTION_ERR (\S+) (.+?) (\S+) err (\S+) bound (\S+)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.log:
        r = subprocess.CompletedProcess([], 0, stdout=Path(a.log).read_text(), stderr="")
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_motion.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"], cwd=str(REPO),
                           capture_output=True, text=True, timeout=600)
    rows = [m.groups() for m in LINE.finditer(r.stdout)]
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("motion_errors.py: the GPU tests printed no figures (no MI355X?)")
    worst, count = {}, {}
    for kind, case, crit, err, bound in rows:
        crit = crit if kind != "flow" or not case.split()[-1].startswith("chunk") else f"{crit} (per chunk)"
        key = (kind, crit)
        count[key] = count.get(key, 0) + 1
        err, bound = float(err), float(bound)
        share = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if key not in worst or share > worst[key][0]:
            worst[key] = (share, case, err, bound)
    exact = [ln.strip().lstrip(".") for ln in r.stdout.splitlines() if "not bit-equal" in ln or "triples that differ" in ln]
    tail = r.stdout.strip().splitlines()[-1]
    lines = ["Video motion forensics on the MI355X (tests/test_gpu_motion.py): ChronosGuard's statistics, the pyramid chunks' mean and std of the per-pixel",
             "mean |d|, both normalised vectors and cache_visual against the mirror's float64 evaluation on the device's own per-pair series and gray",
             "planes.  Worst case per quantity over every clip of the run, as err / bound; the bounds are those of the reference's float32 NumPy",
             "arithmetic (tests/motion_ref.py), the device evaluates in double and rounds once.  A bound of 0 marks a quantity that is exact (max).",
             "Gray planes, flow magnitudes, 8-bin counts, chunk maxima and NaN positions are compared bit for bit by the tests and have no row here.", ""]
    for (kind, crit), (share, case, err, bound) in sorted(worst.items()):
        lines.append(f"  {kind:13s} {crit:22s} {share:9.5f}   at {case} (err {err:.3e}, bound {bound:.3e}; {count[(kind, crit)]} figures)")
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
