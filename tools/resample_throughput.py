#!/usr/bin/env python3
"""Throughput of the device resampler (ultrafnd_git_amd/audio.py: resample, csrc/resample.hip) on one MI355X: one process, one
GPU, unprofiled, clips resident on the device.

    resample_throughput.py [--out profiles/resample_throughput.txt]
        B = 32 x 1-s and B = 32 x 5-s clips, 44.1 kHz -> 16 kHz and 48 kHz -> 16 kHz, at the three qualities, mono fp32; stereo int16
        against mono fp32 at 44.1 kHz kaiser_best.  Beside each time, counted from the shapes and the tap tables by this file:
          useful MACs   sum of count[p] per n outputs (the stored bands)
          issued MACs   what the kernel executes: the group bands (union of 4 phases, rounded to 8 taps), 4 phases per group, 64
                        lanes per wave for every tile the clip reaches
          bytes         samples read once + outputs written once, and the time they would take at the guide's HBM rate
          share         useful FLOP (2 per MAC) over the call time, as a share of the fp32 vector peak the microarchitecture guide
                        states (157.3 TF; recalled, not measured here).  The kernel is a VALU FIR (v_pk_fma_f32), not an MFMA kernel.
        The call time of the plain calls holds the host's enqueue work (one launch, two allocations); the replayed hipGraph's time
        is the kernel's own.
        Baseline on the same device and inputs: the same filter as torch.nn.functional.conv1d(pad(x), h.view(n, 1, K), stride=o) in
        fp32, the dense formulation (every phase over all K taps), its outputs compared with the kernel's.
        And cache_audio(sr=44100) against cache_audio on the same seconds of 16 kHz audio: the stage's share of the end-to-end call.

Device events around windows of >= 0.5 s after warm-up, three windows per path, the paths alternated; median.  Run it under a `timeout`.
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch
import torch.nn.functional as F

from ultrafnd_git_amd import _lib as L
from ultrafnd_git_amd import audio

VECTOR_F32_PEAK, HBM_PEAK = 157.3e12, 8.0e12
B = 32

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


def counts(t, n_in, channels=1, in_bytes=4):
    """(useful MACs, issued MACs, bytes) of one clip of n_in samples."""
    o, n, G = t["o"], t["n"], t["G"]
    m = audio.resampled_length(n_in, t["orig_sr"], t["new_sr"])
    useful = sum(int(t["count"][j % n]) for j in range(m))
    tiles = -(-m // t["out_tile"])
    issued = tiles * t["qt"] * 4 * int(t["groups"][:, 1].sum())
    return useful, issued, n_in * channels * in_bytes + m * 4


def conv1d_baseline(x, t, h):
    """The dense formulation: every phase over all K taps; (B, n, Q) -> (B, Q n) cut to m_max."""
    o, n, width, K = t["o"], t["n"], t["width"], t["K"]
    m = audio.resampled_length(x.shape[1], t["orig_sr"], t["new_sr"])
    q = -(-m // n)
    pad_r = max(0, (q - 1) * o + K - width - x.shape[1])
    y = F.conv1d(F.pad(x[:, None, :], (width, pad_r)), h, stride=o)[:, :, :q]
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :m]


if not torch.cuda.is_available():
    raise SystemExit("resample_throughput.py measures on a GPU: none found (no CPU fallback)")
dev = torch.device("cuda")
say(f"# audio.resample on {torch.cuda.get_device_name(0)}; device events, windows >= {a.window} s, median of 3, paths alternated; B = {B}, clips resident")
say(f"# share = useful FLOP / time / {VECTOR_F32_PEAK / 1e12:.1f} TF (the guide's fp32 vector peak, not measured here); HBM floor = bytes / {HBM_PEAK / 1e12:.1f} TB/s (spec)")
for orig in (44100, 48000):
    for seconds in (5, 1):
        n_in = orig * seconds
        g = torch.Generator(device="cpu").manual_seed(orig + seconds)
        x = (0.1 * torch.randn(B, n_in, generator=g)).to(dev)
        say(f"{orig} Hz -> 16000 Hz, {B} x {seconds}-s clips ({n_in} samples), mono fp32:")
        for q in audio.RESAMPLE_QUALITIES:
            t = audio.resample_taps(orig, 16000, q)
            h = torch.from_numpy(t["h"]).to(dev).view(t["n"], 1, t["K"])
            useful, issued, nbytes = (B * v for v in counts(t, n_in))
            ours = audio.resample(x, None, orig_sr=orig, quality=q)["waves"]
            theirs = conv1d_baseline(x, t, h)
            diff = float((ours - theirs).abs().max())
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                held = audio.resample(x, None, orig_sr=orig, quality=q)
            paths = {"resample (plain call)": lambda: audio.resample(x, None, orig_sr=orig, quality=q),
                     "resample (replayed hipGraph: device time)": graph.replay,
                     "conv1d baseline (dense, all K taps)": lambda: conv1d_baseline(x, t, h)}
            ms = {k: [] for k in paths}
            for _ in range(3):
                for k, fn in paths.items():
                    ms[k].append(timed(fn, a.window))
            say(f"  {q}: o/n = {t['o']}/{t['n']}, K = {t['K']}, G = {t['G']}, tile = {t['out_tile']} outputs; useful {useful / 1e6:.1f} MMAC, issued "
                f"{issued / 1e6:.1f} MMAC ({100.0 * useful / issued:.0f} % useful), dense {B * audio.resampled_length(n_in, orig) * t['K'] / 1e6:.1f} MMAC; "
                f"{nbytes / 1e6:.1f} MB in + out = {nbytes / HBM_PEAK * 1e3:.4f} ms at HBM peak; max |kernel - conv1d| = {diff:.2e}")
            for k, v in ms.items():
                m = statistics.median(v)
                share = "" if "conv1d" in k else f"  {2 * useful / (m * 1e-3) / 1e12:6.2f} TF useful = {100.0 * 2 * useful / (m * 1e-3) / VECTOR_F32_PEAK:4.1f} % of the fp32 vector peak"
                say(f"    {k:44s} {m:8.4f} ms/call  {B / (m * 1e-3):9.0f} clips/s  (windows {min(v):.4f} .. {max(v):.4f}){share}")
            del graph, held

# stereo int16 (a decoder's channel-last PCM buffer, read in place) against mono fp32
n_in = 44100 * 5
g = torch.Generator(device="cpu").manual_seed(3)
pcm = torch.randint(-32768, 32768, (B, n_in, 2), generator=g, dtype=torch.int16).to(dev)
mono = (pcm.float().mean(dim=2) / 32768.0).contiguous()
say(f"44100 Hz -> 16000 Hz kaiser_best, {B} x 5-s clips: stereo int16 channel-last (read through its strides, scale 1/32768) against mono fp32:")
paths = {"stereo int16 (B, n, 2) viewed as (B, 2, n)": lambda: audio.resample(pcm.permute(0, 2, 1), None, orig_sr=44100, scale=1.0 / 32768.0),
         "mono fp32": lambda: audio.resample(mono, None, orig_sr=44100)}
ms = {k: [] for k in paths}
for _ in range(3):
    for k, fn in paths.items():
        ms[k].append(timed(fn, a.window))
for k, v in ms.items():
    m = statistics.median(v)
    say(f"    {k:44s} {m:8.4f} ms/call  {B / (m * 1e-3):9.0f} clips/s  (windows {min(v):.4f} .. {max(v):.4f})")

# the stage's share of the end-to-end cache call
x441 = (0.1 * torch.randn(B, 44100 * 5, generator=g)).to(dev)
x16 = (0.1 * torch.randn(B, 16000 * 5, generator=g)).to(dev)
say(f"cache_audio, {B} x 5-s clips (features of the STFT branch):")
paths = {"cache_audio(x, sr=44100)  (resample + STFT)": lambda: audio.cache_audio(x441, None, 128, sr=44100),
         "cache_audio(x)  (16 kHz audio, STFT only)": lambda: audio.cache_audio(x16, None, 128)}
ms = {k: [] for k in paths}
for _ in range(3):
    for k, fn in paths.items():
        ms[k].append(timed(fn, a.window))
for k, v in ms.items():
    m = statistics.median(v)
    say(f"    {k:44s} {m:8.4f} ms/call  {B / (m * 1e-3):9.0f} clips/s  (windows {min(v):.4f} .. {max(v):.4f})")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
