#!/usr/bin/env python3
"""The record of tests/test_gpu_audio.py: the audio encoder's measured error against the float64 yardstick, as a ratio to the
bf16-operand mirror's own error on the same input (bf16 stages; the tests allow 3) or to the rounding bound (fp32-only stages; the
tests allow 1).  Runs the test file in a child process on the MI355X and collects the figures every test prints before it asserts.

    python tools/audio_errors.py [--out profiles/audio_errors.txt] [--log FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_audio.py -m gpu -s` run on the MI355X instead of running one.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LINE = re.compile(r"AUDIO_ERR (\S+) (\S+) gpu=(\S+) bound=(\S+) (ratio_to_mirror|ratio_to_bound)=(\S+)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.log:
        r = subprocess.CompletedProcess([], 0, stdout=Path(a.log).read_text(), stderr="")
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_audio.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"], cwd=str(REPO),
                           capture_output=True, text=True, timeout=900)
    rows = [m.groups() for m in LINE.finditer(r.stdout)]
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("audio_errors.py: the GPU tests printed no figures (no MI355X?)")
    worst = {}
    for name, crit, gpu, bound, kind, ratio in rows:
        case, stage = name.rsplit(".", 1)
        k = (kind, stage, crit)
        if k not in worst or float(ratio) > worst[k][0]:
            worst[k] = (float(ratio), case, float(gpu), float(bound))
    bits = re.findall(r"AUDIO_BITS (\S+) hidden_equal=(\S+) feature_equal=(\S+)", r.stdout)
    tail = r.stdout.strip().splitlines()[-1]
    lines = ["audio encoder on the MI355X against transformers.Wav2Vec2Model in float64, one clip at a time (tests/test_gpu_audio.py; layers = 2",
             "per stage, 12 for full12): worst case per stage and criterion", "",
             "bf16 stages: GPU error / the bf16-operand mirror's own error on the same input (the tests hold every case to 3)"]
    for (kind, stage, crit), (ratio, case, gpu, bound) in sorted(worst.items()):
        if kind == "ratio_to_mirror":
            lines.append(f"  {stage:10s} {crit:14s} {ratio:6.2f}   at {case} (gpu {gpu:.3e}, bound {bound:.3e})")
    lines += ["", "fp32-only stages: GPU max-abs error / rounding bound of tests/audio_ref.py FP32_BOUNDS (the tests hold every case to 1)"]
    for (kind, stage, crit), (ratio, case, gpu, bound) in sorted(worst.items()):
        if kind == "ratio_to_bound":
            lines.append(f"  {stage:10s} {crit:14s} {ratio:6.2f}   at {case} (gpu {gpu:.3e}, bound {bound:.3e})")
    lines += ["", "a clip inside the mixed batch against the same clip alone (bit comparison of hidden state and feature)"]
    lines += [f"  {n:10s} hidden_equal={h} feature_equal={f}" for n, h, f in bits]
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
