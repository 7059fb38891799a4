#!/usr/bin/env python3
"""Measured figures of the resampler (ultrafnd_git_amd/audio.py: resample, csrc/resample.hip) against tests/resample_ref.py.

    resample_errors.py [--out profiles/resample_errors.txt] [--filter-only]
        filter (float64 mirror, no device): per rate -> 16 kHz and quality the worst |phase DC sum - 1|, the gains of 1 kHz and
            3 kHz tones and the residual of a tone 2 kHz above the lower Nyquist frequency (0.05 s, RMS x sqrt 2 over the middle half)
        kernel (on a GPU): per rate pair and quality, seeded 0.1 randn clips at the edge lengths of tests/test_gpu_resample.py: the
            worst |y - y64| / ((T_p + 1) 2^-24 sum |h| |x|) (<= 1 passes), the relative L2 to float64 of the kernel and of the
            float32 mirror of the declared chain order, and how many values differ from that mirror
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np
import torch

import resample_ref as R
from ultrafnd_git_amd import audio

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--filter-only", action="store_true")
a = ap.parse_args()
if not a.filter_only and not torch.cuda.is_available():
    raise SystemExit("resample_errors.py measures the kernel on a GPU: none found (no CPU fallback; --filter-only for the host figures)")
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


say("# filter figures on the float64 mirror with the fp32-rounded taps (host only)")
say(f"{'rate':>6s} {'quality':12s} {'|DC - 1|':>10s} {'gain 1 kHz':>12s} {'gain 3 kHz':>12s} {'alias tone':>11s} {'residual':>10s}")
for sr in R.PAIRS_TO_16K:
    for q in R.QUALITIES:
        ref = R.taps_ref(sr, 16000, q)
        dc = float(np.abs(ref["h"].astype(np.float64).sum(axis=1) - 1.0).max())
        f = 0.5 * min(sr, 16000) + 2000.0
        alias = f"{R.tone_gain(ref, sr, f):10.2e}" if f < sr / 2 else f"{'-':>10s}"      # (a source that cannot carry the tone: no figure)
        say(f"{sr:6d} {q:12s} {dc:10.2e} {R.tone_gain(ref, sr, 1000.0):12.9f} {R.tone_gain(ref, sr, 3000.0):12.9f} {f:9.0f} Hz {alias}")

if not a.filter_only:
    say(f"# audio.resample on {torch.cuda.get_device_name(0)} against the float64 mirror; ratio = |y - y64| / ((T_p + 1) 2^-24 sum |h| |x|) (<= 1 passes)")
    say(f"{'pair':>14s} {'quality':12s} {'clips':>5s} {'worst ratio':>11s} {'relL2 kernel':>12s} {'relL2 chain':>12s} {'differ from chain':>18s}")
    rng = np.random.default_rng(2026)
    for orig, new in R.PAIRS:
        for q in R.QUALITIES:
            t, ref = audio.resample_taps(orig, new, q), R.taps_ref(orig, new, q)
            o, width = t["o"], t["width"]
            lens = sorted({1, max(width, 1), 3 * o - 1, 3 * o, 3 * o + 1, 2500 + o})
            clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
            batch = torch.full((len(clips), max(lens)), float("nan"))
            for r, x in enumerate(clips):
                batch[r, :len(x)] = torch.from_numpy(x)
            y = audio.resample(batch.cuda(), lens, orig_sr=orig, new_sr=new, quality=q)["waves"].cpu().numpy()
            worst = 0.0
            for r, x in enumerate(clips):
                y64, bound = R.resample_ref(x, ref)
                worst = max(worst, float((np.abs(y[r, :len(y64)] - y64) / bound).max()))
            chain = R.resample_chain_f32(clips[-1], ref)
            mine, norm = y[-1, :len(y64)], np.linalg.norm(y64)
            say(f"{orig:6d}->{new:6d} {q:12s} {len(clips):5d} {worst:11.4f} {np.linalg.norm(mine - y64) / norm:12.3e} {np.linalg.norm(chain - y64) / norm:12.3e} "
                f"{int((mine != chain).sum()):8d} of {len(y64):6d}")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
