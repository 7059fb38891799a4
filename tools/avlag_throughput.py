#!/usr/bin/env python3
"""Throughput of batched A/V lag estimation (ultrafnd_git_amd/temporal.py: av_lag) on one MI355X: one process, one GPU, unprofiled,
envelopes resident on the device.

    avlag_throughput.py [--out profiles/avlag_throughput.txt]
        B = 32 pairs at  n = 125, K = 124 (5 s at 25 fps, the full window),  n = 4000, K = 2000  and  n = 80000, K = 8000 (a 5-s
        envelope at audio rate): ms per call of av_lag(want=("lag_seconds",)) and, alternated with it in the same process,
          (a) a torch.fft composition of the same window on the device (standardise, rfft of the first power of two >= 2 n,
              product with the conjugate, irfft, the window's columns, argmax) -- fp32, as the reference's FFT is under NumPy 2;
          (b) the package's own host TemporalSyncNet.estimate_av_lag called B times on NumPy rows (the reference's call pattern;
              host clock, three repeats, no device involved).
        The useful multiply-adds of the direct form, sum over the window's lags of (n - |k|), are printed with the rate they imply
        over the call time (a whole-call figure, not a kernel's share of peak).  The agreement of (a) with av_lag is printed too.

Device events around windows of >= 0.3 s after warm-up, three windows per path, the paths alternated; median.  Run it under a `timeout`.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from ultrafnd_git_amd import temporal

SHAPES = ((32, 125, 124), (32, 4000, 2000), (32, 80000, 8000))      # B, n, K  (sr = 1: K = int(max_lag_s))

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
    n = 2
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


def torch_fft_lag(x, y, K):
    """The reference's algorithm on the device: (B,) lags in samples."""
    n = x.shape[1]
    xs = (x - x.mean(1, keepdim=True)) / (x.std(1, unbiased=False, keepdim=True) + 1e-9)
    ys = (y - y.mean(1, keepdim=True)) / (y.std(1, unbiased=False, keepdim=True) + 1e-9)
    nfft = 1
    while nfft < 2 * n:
        nfft <<= 1
    xc = torch.fft.irfft(torch.fft.rfft(xs, nfft) * torch.conj(torch.fft.rfft(ys, nfft)), nfft)
    Kc = min(K, n - 1)
    win = torch.cat([xc[:, nfft - Kc:], xc[:, :Kc + 1]], dim=1)      # lags -Kc .. Kc
    return win.argmax(1) - Kc


if not torch.cuda.is_available():
    raise SystemExit("avlag_throughput.py measures on a GPU: none found (no CPU fallback)")
dev = torch.device("cuda")
say(f"# av_lag on {torch.cuda.get_device_name(0)}; device events, windows >= {a.window} s, median of 3, paths alternated; B = 32")
for B, n, K in SHAPES:
    rng = np.random.default_rng(B + n)
    base = np.convolve(rng.standard_normal((B, n + 2 * K + 2)).ravel(), [0.25, 0.5, 0.25], "same").reshape(B, -1)
    shifts = rng.integers(-min(K, n // 4), min(K, n // 4) + 1, B)
    m_h = (0.6 + 0.25 * base[:, K:K + n]).astype(np.float32)
    a_h = np.stack([1.0 + 0.2 * base[b, K - s:K - s + n] for b, s in enumerate(shifts)]).astype(np.float32) + (0.02 * rng.standard_normal((B, n))).astype(np.float32)
    x, y = torch.from_numpy(a_h).to(dev), torch.from_numpy(m_h).to(dev)
    Kc = min(K, n - 1)
    macs = B * sum(n - abs(k) for k in range(-Kc, Kc + 1))
    paths = {
        "av_lag(want=('lag_seconds',)): direct window": lambda: temporal.av_lag(x, y, None, None, 1.0, 25.0, float(K), ("lag_seconds",)),
        "(a) torch.fft composition of the same window": lambda: torch_fft_lag(x, y, K),
    }
    ours = temporal.av_lag(x, y, None, None, 1.0, 25.0, float(K), ("lag_samples",))["lag_samples"].cpu().numpy()
    fft = torch_fft_lag(x, y, K).cpu().numpy()
    say(f"n = {n}, K = {K} ({2 * Kc + 1} lags): {macs / 1e9:.3f} G useful multiply-adds per call; lags equal to the planted shifts: av_lag "
        f"{int((ours == shifts).sum())} / {B}, torch.fft {int((fft == shifts).sum())} / {B}; av_lag = torch.fft on {int((ours == fft).sum())} / {B} pairs")
    ms = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():
            ms[k].append(timed(fn, a.window))
    for k, v in ms.items():
        med = statistics.median(v)
        rate = f"  {macs / (med * 1e-3) / 1e12:6.2f} T multiply-adds/s over the call" if k.startswith("av_lag") else ""
        say(f"  {k:50s} {med:9.4f} ms/call  {B / (med * 1e-3):10.0f} pairs/s  (windows {min(v):.4f} .. {max(v):.4f}){rate}")
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = [temporal.TemporalSyncNet.estimate_av_lag(a_h[b], m_h[b], sr=1.0, max_lag_s=float(K)) for b in range(B)]
        host.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(host)
    say(f"  {'(b) host estimate_av_lag x ' + str(B) + ' (NumPy, host clock)':50s} {med:9.4f} ms/call  {B / (med * 1e-3):10.0f} pairs/s  (repeats {min(host):.4f} .. "
        f"{max(host):.4f}); lags equal to the planted shifts: {int((np.array(got) == shifts).sum())} / {B}")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
