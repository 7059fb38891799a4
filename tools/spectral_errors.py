#!/usr/bin/env python3
"""Measured error of the STFT audio forensics against the float64 mirror (tests/spectral_ref.py), as a ratio to each derived bound
and to the float32 mirror of the kernel's own summation order, per output and per fixture clip.

    spectral_errors.py [--out profiles/spectral_errors.txt]
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np
import torch

import spectral_ref as R
from ultrafnd_git_amd import audio

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("spectral_errors.py measures on a GPU: none found (no CPU fallback)")
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


say(f"# stft_forensics on {torch.cuda.get_device_name(0)} against the float64 mirror; ratio = measured error / derived bound (<= 1 passes)")
say("# chain = relative L2 of the magnitudes against float64 over that of the float32 chain mirror (<= 3 passes); ref = the reference's own fp32 values")
say(f"{'clip':12s} {'T':>4s} {'magnitude':>10s} {'mel_like':>9s} {'mean':>8s} {'std':>8s} {'max':>8s} {'min':>8s} {'features':>9s} {'score':>8s} {'chain':>6s} {'relL2':>9s} {'ref mag':>8s}")
basis32 = audio.dft_basis()
ratio = lambda d, b: float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0))))
for name, g in R.golden().items():
    x = R.mono(g["wave"])
    mag, T = R.magnitude64(x), R.frame_count(len(x))
    st = R.stats64(mag)
    sb = R.stats_bound(x, st)
    d = R.bin_bound(x)[None, :]
    o = {k: v.cpu().numpy()[0] for k, v in audio.stft_forensics(torch.from_numpy(x)[None].cuda(), None, 128, ("features", "stats", "mel_like", "magnitude")).items()}
    e = R.energy64(x)
    sc = float(audio.wave_energy(torch.from_numpy(x)[None].cuda())["score"][0].cpu())
    chain = R.rel_l2(R.chain_magnitude32(x, basis32), mag)
    mine = R.rel_l2(o["magnitude"][:, :T], mag)
    rs = [abs(float(o["stats"][k]) - st[k]) / sb[k] if sb[k] > 0 else 0.0 for k in range(4)]
    refmag = ratio(np.abs(g["magnitude"].astype(np.float64) - mag), d) if "magnitude" in g else float("nan")
    sbd = R.score_bound(len(x), e)
    say(f"{name:12s} {T:4d} {ratio(np.abs(o['magnitude'][:, :T] - mag), d):10.4f} {ratio(np.abs(o['mel_like'][:, :T] - R.mel64(mag)), R.mel_bound(x, R.mel64(mag))):9.4f} "
        f"{rs[0]:8.4f} {rs[1]:8.4f} {rs[2]:8.4f} {rs[3]:8.4f} {ratio(np.abs(o['features'] - R.features64(st, 128)), R.features_bound(st, sb, 128)):9.4f} "
        f"{(abs(sc - R.score64(e)) / sbd if sbd > 0 else 0.0):8.4f} {(mine / chain if chain > 0 else 0.0):6.3f} {mine:9.2e} {refmag:8.4f}")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
