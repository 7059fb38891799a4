#!/usr/bin/env python3
"""Throughput of the STFT audio forensics (ultrafnd_git_amd/audio.py: stft_forensics) on one MI355X: one process, one GPU,
unprofiled, clips resident on the device.

    spectral_throughput.py [--out profiles/spectral_throughput.txt]
        B = 32 x 1-s and B = 32 x 5-s clips (16 kHz): ms per call and clips/s of the statistics-only call (features + stats), the
        statistics + mel_like call and the full call (+ magnitude); the DFT GEMM's operations (2 x 402 x 400 per frame) over the call
        time as a share of the fp32-MFMA peak the microarchitecture guide states (157.3 TF; recalled, not measured here).  The call
        time of the plain calls holds the host's enqueue work (two launches, the output allocations), so their share is an end-to-end
        figure; the replayed graph's is the two kernels' own.
        Yardsticks on the same device and inputs: torch.stft(n_fft=400, hop_length=160).abs() followed by torch reductions (mean, std,
        amax, amin per clip, tiled and normalised), batched; and the reference-style loop, one clip per call of the same composition
        with the four statistics brought to the host, as the reference does.

Device events around windows of >= 0.5 s after warm-up, three windows per path, the paths alternated; median.  Run it under a `timeout`.
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

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--window", type=float, default=0.5)
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


def torch_stats(x, dim=128):
    mag = torch.stft(x, n_fft=400, hop_length=160, window=WINDOW, return_complex=True).abs()
    st = torch.stack([mag.mean(dim=(1, 2)), mag.std(dim=(1, 2), unbiased=False), mag.amax(dim=(1, 2)), mag.amin(dim=(1, 2))], dim=1)
    v = st.repeat(1, dim // 4)
    return v / (torch.linalg.vector_norm(v, dim=1, keepdim=True) + 1e-9)


def reference_style_loop(x, dim=128):
    rows = []
    for b in range(x.shape[0]):
        mag = torch.stft(x[b], n_fft=400, hop_length=160, window=WINDOW, return_complex=True).abs()
        rows.append(torch.stack([mag.mean(), mag.std(unbiased=False), mag.max(), mag.min()]).cpu())
    return rows


if not torch.cuda.is_available():
    raise SystemExit("spectral_throughput.py measures on a GPU: none found (no CPU fallback)")
dev = torch.device("cuda")
WINDOW = torch.ones(400, device=dev)
say(f"# stft_forensics on {torch.cuda.get_device_name(0)}; device events, windows >= {a.window} s, median of 3, paths alternated")
say(f"# share of peak = 2 x 402 x 400 FLOP per frame / call time / {MFMA_F32_PEAK / 1e12:.1f} TF (the guide's fp32-MFMA peak, not measured here)")
for B, n in SHAPES:
    g = torch.Generator(device="cpu").manual_seed(B + n)
    x = (0.1 * torch.randn(B, n, generator=g)).to(dev)
    T = 1 + n // 160
    flop = 2.0 * 402 * 400 * T * B
    paths = {
        "stats only (features + stats)": lambda: audio.stft_forensics(x, None, 128, ("features", "stats")),
        "stats + mel_like": lambda: audio.stft_forensics(x, None, 128, ("features", "stats", "mel_like")),
        "stats + mel_like + magnitude": lambda: audio.stft_forensics(x, None, 128, ("features", "stats", "mel_like", "magnitude")),
        "torch.stft().abs() + torch reductions, batched": lambda: torch_stats(x),
        "reference-style loop (batch 1, stats to the host)": lambda: reference_style_loop(x),
    }
    # the statistics-only call captured into a hipGraph: the replay takes the host's enqueue work out of the time
    audio.stft_forensics(x, None, 128)      # (the basis is uploaded on the first call: not inside a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = audio.stft_forensics(x, None, 128, ("features", "stats"))
    paths["stats only, replayed hipGraph (device time)"] = graph.replay
    ours, theirs = audio.stft_forensics(x, None, 128)["features"], torch_stats(x)
    say(f"B = {B} x {n} samples ({n / 16000:g} s): {T} frames per clip, {flop / 1e9:.2f} GFLOP as a DFT GEMM; "
        f"max |features - torch composition| = {float((ours - theirs).abs().max()):.2e}")
    ms = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():
            ms[k].append(timed(fn, a.window))
    for k, v in ms.items():
        m = statistics.median(v)
        share = f"  {flop / (m * 1e-3) / 1e12:6.1f} TF = {100.0 * flop / (m * 1e-3) / MFMA_F32_PEAK:4.1f} % of the fp32-MFMA peak" if "torch" not in k and "loop" not in k else ""
        say(f"  {k:52s} {m:8.4f} ms/call  {B / (m * 1e-3):10.0f} clips/s  (windows {min(v):.4f} .. {max(v):.4f}){share}")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
