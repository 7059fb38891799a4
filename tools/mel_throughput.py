#!/usr/bin/env python3
"""Throughput of the librosa-branch mel spectrogram in dB (ultrafnd_git_amd/audio.py: mel_spectrogram) on one MI355X: one process,
one GPU, unprofiled, clips resident on the device.

    mel_throughput.py [--out profiles/mel_throughput.txt] [--errors profiles/mel_errors.txt]
        B = 32 x 5-s and B = 32 x 1-s clips (16 kHz): ms per call and clips/s of mel_spectrogram(want=("mel_db",)), and in the same
        process, alternated with it:
          (a) spectral_descriptors(want=("magnitude",)): the same STFT tile without the mel and dB stages.  It is not a pure floor:
              that kernel stores the (201, T) magnitudes and always runs the descriptors' per-frame epilogue (band peaks and
              valleys, the flatness and the tile statistics in double), one launch against the mel call's two;
          (b) a torch composition on the device: torch.stft with the Hann window (center=True, pad_mode="constant"), abs() ** 2, a
              matmul with the (64, 201) weights, then log10, the per-clip maximum and the clamp.
        The torch composition is also an independent device check: its largest disagreement with mel_db is printed (and written to
        --errors).

Device events around windows of >= 0.3 s after warm-up, three windows per path, the paths alternated; median.  Run it under a `timeout`.
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from ultrafnd_git_amd import audio

SHAPES = ((32, 80000), (32, 16000))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--errors", default=None)
ap.add_argument("--window", type=float, default=0.3)
a = ap.parse_args()
out, errs = [], []


def say(s, also=None):
    print(s, flush=True)
    out.append(s)
    if also is not None:
        also.append(s)


def timed(fn, window):
    """ms per call: calls are enqueued between two device events until the window is filled."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 4
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= window * 1000.0:
            return ms / n
        n = max(n * 2, int(n * window * 1000.0 / max(ms, 1e-3)) + 1)


def torch_mel_db(x):
    S = torch.stft(x, n_fft=400, hop_length=160, window=WIN, center=True, pad_mode="constant", return_complex=True).abs()
    M = torch.matmul(W, S * S)
    L = 10.0 * torch.log10(M.clamp_min(1e-10))
    L = L - L.amax(dim=(1, 2), keepdim=True)
    return L.clamp_min(-80.0)


if not torch.cuda.is_available():
    raise SystemExit("mel_throughput.py measures on a GPU: none found (no CPU fallback)")
dev = torch.device("cuda")
WIN = torch.hann_window(400, periodic=True, device=dev)
W = torch.from_numpy(audio.mel_filterbank()["weights"].copy()).to(dev)
say(f"# mel_spectrogram on {torch.cuda.get_device_name(0)}; device events, windows >= {a.window} s, median of 3, paths alternated")
for B, n in SHAPES:
    g = torch.Generator(device="cpu").manual_seed(B + n)
    x = (0.1 * torch.randn(B, n, generator=g)).to(dev)
    T = 1 + n // 160
    paths = {
        "mel_spectrogram(want=('mel_db',))": lambda: audio.mel_spectrogram(x, None, ("mel_db",)),
        "(a) spectral_descriptors(want=('magnitude',)): the same STFT tile": lambda: audio.spectral_descriptors(x, None, 128, ("magnitude",)),
        "(b) torch composition (stft, |.|^2, matmul, log10, max, clamp)": lambda: torch_mel_db(x),
    }
    ours, theirs = audio.mel_spectrogram(x, None, ("mel_db",))["mel_db"], torch_mel_db(x)
    say(f"B = {B} x {n} samples ({n / 16000:g} s): {T} frames per clip; max |mel_db - torch composition| = "
        f"{float((ours - theirs).abs().max()):.2e} dB", errs)
    ms = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():
            ms[k].append(timed(fn, a.window))
    for k, v in ms.items():
        m = statistics.median(v)
        say(f"  {k:68s} {m:8.4f} ms/call  {B / (m * 1e-3):10.0f} clips/s  (windows {min(v):.4f} .. {max(v):.4f})")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
if a.errors:
    Path(a.errors).parent.mkdir(parents=True, exist_ok=True)
    Path(a.errors).write_text("\n".join(errs) + "\n")
