#!/usr/bin/env python3
"""The record of tests/test_gpu_encoder_geometry.py: the four frozen encoders' measured error against their float64 yardsticks at every
geometry of tests/encoder_geometry_cases.py, as a ratio to the bf16-operand mirror's own error on the same input (bf16 stages; the
tests allow 3) or to the rounding bound (the text towers' fp32 embeddings; the tests allow 1), and the bit comparisons.  Runs the test
file in a child process on the MI355X and collects the figures every test prints before it asserts.

    python tools/encoder_geometry_errors.py [--out profiles/encoder_geometry_errors.txt] [--log FILE] [--note FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_encoder_geometry.py -m gpu -s` run on the MI355X instead of
running one.  --note FILE: text appended to the record (the explanation a ratio to the mirror above 2 calls for).
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LINE = re.compile(r"ENC_GEOM_ERR (\S+) (\S+) (\S+) gpu=(\S+) bound=(\S+) (ratio_to_mirror|ratio_to_bound)=(\S+)")
BITS = re.compile(r"ENC_GEOM_BITS (\S+) (.*)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    if a.log:
        r = subprocess.CompletedProcess([], 0, stdout=Path(a.log).read_text(), stderr="")
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_encoder_geometry.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"],
                           cwd=str(REPO), capture_output=True, text=True, timeout=1800)
    rows = [m.groups() for m in LINE.finditer(r.stdout)]
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("encoder_geometry_errors.py: the GPU tests printed no figures (no MI355X?)")
    worst, order = {}, []
    for case, stage, crit, gpu, bound, kind, ratio in rows:
        ratio = float(gpu) / float(bound) * (3.0 if kind == "ratio_to_mirror" else 1.0) if float(bound) > 0 else float(ratio)
        k = (case, stage.split(".")[0])      # (feature.packed / feature.padded, logits.packed / ...: one line per stage)
        if k not in worst:
            order.append(k)
        if k not in worst or ratio > worst[k][0]:
            worst[k] = (ratio, crit, float(gpu), float(bound), kind, stage)
    tail = [ln for ln in r.stdout.strip().splitlines() if " passed" in ln or " failed" in ln][-1:]
    lines = ["The frozen encoders on the MI355X at every geometry of tests/encoder_geometry_cases.py against float64 (2 layers; BERT and the ViT:",
             "oracle/encoders_ref in float64; RoBERTa and the CLIP text tower: the installed transformers classes in float64), from",
             "tests/test_gpu_encoder_geometry.py: the worst criterion per case and stage.",
             "  ratio_to_mirror  GPU error / the bf16-operand mirror's own error on the same input, in the form the case takes (the tests hold 3)",
             "  ratio_to_bound   share of the fp32 rounding bound that was needed (the text towers' embeddings; the tests hold 1)", ""]
    last = None
    for case, stage in order:
        ratio, crit, gpu, bound, kind, full = worst[(case, stage)]
        if case != last:
            lines.append(case)
            last = case
        lines.append(f"  {stage:14s} {kind:15s} {ratio:7.3f}   worst on {crit:13s} (gpu {gpu:.3e}, bound {bound:.3e}) at {full}")
    all_ratios = [v[0] for v in worst.values() if v[4] == "ratio_to_mirror"]
    lines += ["", f"largest ratio to the mirror over {len(all_ratios)} case-stages: {max(all_ratios):.3f}", "",
              "bit comparisons (features / logits): every property of every case"]
    bits = BITS.findall(r.stdout)
    bad = [(c, b) for c, b in bits if "False" in b]
    props = sorted({p.split("=")[0] for _, b in bits for p in b.split()})
    lines.append(f"  {len(bits)} cases, properties {', '.join(props)}: " + ("all equal" if not bad else f"{len(bad)} cases differ"))
    lines += [f"  DIFFERS {c}: {b}" for c, b in bad]
    if a.note:
        lines += ["", Path(a.note).read_text().rstrip()]
    lines += ["", "pytest: " + (tail[0] if tail else "?")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    if r.returncode != 0:
        raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
