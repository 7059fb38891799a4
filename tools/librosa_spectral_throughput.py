#!/usr/bin/env python3
"""Throughput of the librosa-branch spectral descriptors (ultrafnd_git_amd/audio.py: spectral_descriptors) on one MI355X: one
process, one GPU, unprofiled, clips resident on the device.

    librosa_spectral_throughput.py [--out profiles/librosa_spectral_throughput.txt]
        B = 32 x 1-s and B = 32 x 5-s clips (16 kHz): ms per call and clips/s of the features-only call and of the call with every
        output; the split of the time: path A alone (flatness: STFT 400 / 160 and its per-frame epilogue), path B alone (centroid:
        the K = 2048 DFT GEMM and the per-frame reduction), the zero-crossing kernel alone; the features-only call replayed from a
        hipGraph (the launches' own time, without the host's enqueue work).  Path B's operations as a DFT GEMM (2 x 2050 x 2048 per
        frame) over its time, as a share of the fp32-MFMA peak the microarchitecture guide states (157.3 TF; recalled, not measured).
        Yardstick on the same device and inputs: a torch composition of the same descriptors, batched -- torch.stft with a Hann
        window (center=True, pad_mode="constant") at both geometries, then torch reductions (statistics, flatness, contrast by
        per-band amin / amax and a 2-element topk for band 5, centroid, rolloff by cumsum, zero crossings by unfold).

Device events around windows of >= 0.3 s after warm-up, three windows per path, the paths alternated; median.  Run it under a `timeout`.
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from ultrafnd_git_amd import audio

MFMA_F32_PEAK = 157.3e12
SHAPES = ((32, 16000), (32, 80000))
BANDS = ((0, 5), (4, 10), (9, 20), (19, 40), (39, 80), (79, 160), (159, 201))      # rows [lo, hi) of spectral_contrast's bands

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--window", type=float, default=0.3)
a = ap.parse_args()
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


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


def _db(v):
    d = 10.0 * torch.log10(v.clamp_min(1e-10))
    return torch.maximum(d, d.amax(dim=(1, 2), keepdim=True) - 80.0)


def _flat(S):
    P = (S * S).clamp_min(1e-10)
    return torch.exp(P.log().mean(dim=1)) / P.mean(dim=1)


def torch_descriptors(x, dim=128):
    SA = torch.stft(x, n_fft=400, hop_length=160, window=WIN[400], center=True, pad_mode="constant", return_complex=True).abs()
    SB = torch.stft(x, n_fft=2048, hop_length=512, window=WIN[2048], center=True, pad_mode="constant", return_complex=True).abs()
    peaks, valleys = [], []
    for k, (lo, hi) in enumerate(BANDS):
        band = SA[:, lo:hi]
        if k == 5:
            peaks.append(band.topk(2, dim=1).values.mean(dim=1))
            valleys.append(band.topk(2, dim=1, largest=False).values.mean(dim=1))
        else:
            peaks.append(band.amax(dim=1))
            valleys.append(band.amin(dim=1))
    sc = _db(torch.stack(peaks, dim=1)) - _db(torch.stack(valleys, dim=1))
    sf = _flat(SA)
    f = torch.arange(1025, device=x.device, dtype=torch.float32) * (16000.0 / 2048.0)
    tot = SB.sum(dim=1)
    cent = (f[None, :, None] * SB).sum(dim=1) / tot.clamp_min(1e-30)
    roll = f[(SB.cumsum(dim=1) >= 0.85 * tot[:, None, :]).float().argmax(dim=1)]
    neg = torch.nn.functional.pad(torch.where(x.abs() <= 1e-10, torch.zeros_like(x), x)[:, None], (1024, 1024), mode="replicate")[:, 0] < 0
    fr = neg.unfold(1, 2048, 512)
    zcr = (fr[:, :, 1:] != fr[:, :, :-1]).float().mean(dim=2)
    d = torch.stack([SA.mean(dim=(1, 2)), SA.std(dim=(1, 2), unbiased=False), SA.amax(dim=(1, 2)), SA.amin(dim=(1, 2)), sc.mean(dim=(1, 2)),
                     sc.std(dim=(1, 2), unbiased=False), sf.mean(dim=1), sf.std(dim=1, unbiased=False), cent.mean(dim=1), roll.mean(dim=1),
                     zcr.mean(dim=1)], dim=1)
    v = d.repeat(1, -(-dim // 11))[:, :dim]
    return v / (torch.linalg.vector_norm(v, dim=1, keepdim=True) + 1e-9)


if not torch.cuda.is_available():
    raise SystemExit("librosa_spectral_throughput.py measures on a GPU: none found (no CPU fallback)")
dev = torch.device("cuda")
WIN = {n: torch.hann_window(n, periodic=True, device=dev) for n in (400, 2048)}
say(f"# spectral_descriptors on {torch.cuda.get_device_name(0)}; device events, windows >= {a.window} s, median of 3, paths alternated")
say(f"# share of peak (path B) = 2 x 2050 x 2048 FLOP per frame / time / {MFMA_F32_PEAK / 1e12:.1f} TF (the guide's fp32-MFMA peak, not measured here)")
for B, n in SHAPES:
    g = torch.Generator(device="cpu").manual_seed(B + n)
    x = (0.1 * torch.randn(B, n, generator=g)).to(dev)
    TA, TB = 1 + n // 160, 1 + n // 512
    flop_b = 2.0 * 2050 * 2048 * TB * B
    paths = {
        "features only": lambda: audio.spectral_descriptors(x, None, 128, ("features",)),
        "every output": lambda: audio.spectral_descriptors(x, None, 128, audio.DESC_OUTPUTS),
        "path A alone (flatness)": lambda: audio.spectral_descriptors(x, None, 128, ("flatness",)),
        "path B alone (centroid)": lambda: audio.spectral_descriptors(x, None, 128, ("centroid",)),
        "zero crossings alone (zcr)": lambda: audio.spectral_descriptors(x, None, 128, ("zcr",)),
        "torch composition (torch.stft x 2 + reductions), batched": lambda: torch_descriptors(x),
    }
    audio.spectral_descriptors(x, None, 128)      # (the bases are uploaded on the first call: not inside a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = audio.spectral_descriptors(x, None, 128, ("features",))
    paths["features only, replayed hipGraph (device time)"] = graph.replay
    ours, theirs = audio.spectral_descriptors(x, None, 128)["features"], torch_descriptors(x)
    say(f"B = {B} x {n} samples ({n / 16000:g} s): {TA} + {TB} frames per clip, path B {flop_b / 1e9:.2f} GFLOP as a DFT GEMM; "
        f"max |features - torch composition| = {float((ours - theirs).abs().max()):.2e}")
    ms = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():
            ms[k].append(timed(fn, a.window))
    for k, v in ms.items():
        m = statistics.median(v)
        share = f"  {flop_b / (m * 1e-3) / 1e12:6.1f} TF = {100.0 * flop_b / (m * 1e-3) / MFMA_F32_PEAK:4.1f} % of the fp32-MFMA peak" if "path B" in k else ""
        say(f"  {k:58s} {m:8.4f} ms/call  {B / (m * 1e-3):10.0f} clips/s  (windows {min(v):.4f} .. {max(v):.4f}){share}")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
