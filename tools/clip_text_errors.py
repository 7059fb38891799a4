#!/usr/bin/env python3
"""The record of tests/test_gpu_clip_text.py: the CLIP text tower's and the semantic analyzer's measured error against their float64
yardsticks, as a ratio to the bf16-operand mirror's own error on the same input (bf16 stages; the tests allow 3) or to the rounding
bound (the attention op alone, fp32-only stages; the tests allow 1).  Runs the test file in a child process on the MI355X and collects
the figures every test prints before it asserts.

    python tools/clip_text_errors.py [--out profiles/clip_text_errors.txt] [--log FILE] [--note FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_clip_text.py -m gpu -s` run on the MI355X instead of running one.
--note FILE: text appended to the record (the explanation a ratio to the mirror above 2 calls for).
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LINE = re.compile(r"CLIP_TEXT_ERR (\S+) (\S+) gpu=(\S+) bound=(\S+) (ratio_to_mirror|ratio_to_bound)=(\S+)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    if a.log:
        r = subprocess.CompletedProcess([], 0, stdout=Path(a.log).read_text(), stderr="")
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_clip_text.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"], cwd=str(REPO),
                           capture_output=True, text=True, timeout=900)
    rows = [m.groups() for m in LINE.finditer(r.stdout)]
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("clip_text_errors.py: the GPU tests printed no figures (no MI355X?)")
    worst = {}
    for name, crit, gpu, bound, kind, ratio in rows:
        group, _, rest = name.partition(".")
        stage = ("full12." if group == "full12" else "") + rest.rsplit(".", 1)[-1] if group in ("stage", "full12") else (group if group == "attn" else name)
        if kind == "ratio_to_bound" and float(bound) > 0:
            ratio = float(gpu) / float(bound)      # (the printed ratio keeps two decimals: the worst-case fp32 bounds need more)
        k = (kind, group, stage, crit)
        if k not in worst or float(ratio) > worst[k][0]:
            worst[k] = (float(ratio), name, float(gpu), float(bound))
    bits = re.findall(r"CLIP_TEXT_BITS (.*)", r.stdout)
    tail = r.stdout.strip().splitlines()[-1]
    lines = ["CLIP text tower and semantic analyzer on the MI355X against transformers.CLIPTextModelWithProjection in float64, the reference's",
             "head and float64 restatements (tests/test_gpu_clip_text.py; 2 layers per stage, 12 for full12): worst case per stage and criterion", "",
             "bf16 stages: GPU error / the bf16-operand mirror's own error on the same input (the tests hold every case to 3)"]
    for (kind, group, stage, crit), (ratio, case, gpu, bound) in sorted(worst.items()):
        if kind == "ratio_to_mirror":
            lines.append(f"  {stage:18s} {crit:14s} {ratio:6.2f}   at {case} (gpu {gpu:.3e}, bound {bound:.3e})")
    lines += ["", "the attention op alone (elementwise, against the bound derived from its roundings) and the fp32-only stages (max-abs against",
              "the rounding bounds of tests/clip_text_ref.py): share of the bound that was needed (the tests hold every case to 1)"]
    for (kind, group, stage, crit), (ratio, case, gpu, bound) in sorted(worst.items()):
        if kind == "ratio_to_bound":
            lines.append(f"  {stage:44s} {crit:12s} {ratio:8.4f}   at {case}")
    lines += ["", "bit comparisons (features): packed against padded, two runs, a sample alone against inside the batch, garbage ids after e(b)"]
    lines += ["  " + b for b in bits]
    if a.note:
        lines += ["", Path(a.note).read_text().rstrip()]
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
