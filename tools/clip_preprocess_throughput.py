#!/usr/bin/env python3
"""Throughput of the CLIP image preprocessing (ultrafnd_git_amd/video.py: clip_preprocess) on one MI355X: one process, one GPU,
unprofiled, decoded uint8 frames resident on the device.

    clip_preprocess_throughput.py [--out profiles/clip_preprocess_throughput.txt]
        B = 32 clips of 8 frames of 720 x 1280, of 1 frame of 256 x 256 and of 8 frames of 1080 x 1920 (HWC): ms per call of
        clip_preprocess(want=("pixel_values",)) and, alternated with it in the same process,
          (a) the torch composition on the same device and inputs: permute / float, F.interpolate(mode="bicubic", antialias=True) to the
              processor's size, crop, rescale and normalise -- with its largest difference from the exact pixel_values;
          (b) on the host, CLIPImageProcessorPil called once per image (the call pattern this replaces; host clock, 8 images, three repeats;
              skipped where transformers or Pillow is not installed).
        Bytes moved = the source bytes the crop needs (rows x_lo .. x_lo + x_span of the rows the vertical taps reach, 3 bytes per pixel)
        plus the fp32 output, per call, over the call time, as a share of the HBM peak (8 TB/s): a whole-call figure.

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
import torch.nn.functional as F

from ultrafnd_git_amd import video

SHAPES = ((32, 8, 720, 1280), (32, 1, 256, 256), (32, 8, 1080, 1920))      # B, T, H, W
HBM_PEAK = 8.0e12      # bytes/s (MI355X, HBM3E)
S = 224

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


def torch_composition(frames, tab, mean, std):
    """permute / float, antialiased bicubic interpolation, crop, rescale, normalise: (B, T, 3, S, S) fp32."""
    B, T, H, W, _ = frames.shape
    h2, w2 = tab["resized"]
    x = frames.view(B * T, H, W, 3).permute(0, 3, 1, 2).float()
    y = F.interpolate(x, size=(h2, w2), mode="bicubic", antialias=True, align_corners=False)
    y = y[:, :, tab["top"]:tab["top"] + S, tab["left"]:tab["left"] + S]
    return ((y * (1.0 / 255.0) - mean) / std).view(B, T, 3, S, S)


if not torch.cuda.is_available():
    raise SystemExit("clip_preprocess_throughput.py measures on a GPU: none found (no CPU fallback)")
dev = torch.device("cuda")
try:
    from PIL import Image
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    proc = CLIPImageProcessorPil()
except Exception as e:      # noqa: BLE001
    proc = None
    say(f"# (b) is not measured: {type(e).__name__}: {e}")
mean = torch.tensor(video.CLIP_MEAN, device=dev).view(1, 3, 1, 1)
std = torch.tensor(video.CLIP_STD, device=dev).view(1, 3, 1, 1)
say(f"# clip_preprocess on {torch.cuda.get_device_name(0)}; device events, windows >= {a.window} s, median of 3, paths alternated; image_size {S}")
for B, T, H, W in SHAPES:
    gen = torch.Generator(device=dev).manual_seed(B * T + H)
    frames = torch.randint(0, 256, (B, T, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    tab = video.clip_resize_tables(H, W, S)
    rows = int((tab["v"]["first"] + tab["v"]["count"]).max() - tab["v"]["first"].min())
    moved = B * T * (rows * tab["x_span"] * 3 + 3 * S * S * 4)
    exact = video.clip_preprocess(frames)["pixel_values"]
    paths = {"clip_preprocess(want=('pixel_values',))": lambda: video.clip_preprocess(frames)}
    note = ""
    try:
        approx = torch_composition(frames, tab, mean, std)
        note = f"; torch composition: largest |difference| from the exact pixel_values {float((approx - exact).abs().max()):.4f} " \
               f"({float((approx != exact).float().mean()) * 100:.1f} % of the values differ)"
        del approx
        paths["(a) torch composition (interpolate bicubic antialias)"] = lambda: torch_composition(frames, tab, mean, std)
    except Exception as e:      # noqa: BLE001
        note = f"; torch composition not available: {type(e).__name__}: {e}"
    say(f"B = {B} x {T} frames of {H} x {W}: tile_rows {tab['tile_rows']}, lds_rows {tab['lds_rows']}, {tab['h']['k'].shape[1]} / {tab['v']['k'].shape[1]} taps; "
        f"{moved / 1e6:.1f} MB moved per call (source rows {rows} x columns {tab['x_span']} of {H} x {W}){note}")
    ms = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():
            ms[k].append(timed(fn, a.window))
    for k, v in ms.items():
        med = statistics.median(v)
        rate = f"  {moved / (med * 1e-3) / 1e12:5.2f} TB/s = {moved / (med * 1e-3) / HBM_PEAK * 100:4.1f} % of HBM peak over the call" if k.startswith("clip_pre") else ""
        say(f"  {k:58s} {med:9.4f} ms/call  {B * T / (med * 1e-3):11.0f} frames/s  (windows {min(v):.4f} .. {max(v):.4f}){rate}")
    if proc is not None:
        imgs = [Image.fromarray(x) for x in frames[0, :1].expand(8, H, W, 3).contiguous().cpu().numpy()] if T == 1 else \
               [Image.fromarray(x) for x in frames[0, :8].cpu().numpy()]
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = [proc(images=im, return_tensors="np")["pixel_values"][0] for im in imgs]
            host.append((time.perf_counter() - t0) * 1e3 / len(imgs))
        med = statistics.median(host)
        same = np.array_equal(np.stack(got[:1]).view(np.uint32), exact[0, :1].cpu().numpy().view(np.uint32))
        say(f"  {'(b) host CLIPImageProcessorPil per image (host clock)':58s} {med * B * T:9.4f} ms/call  {1e3 / med:11.0f} frames/s  (per image {min(host):.3f} .. "
            f"{max(host):.3f} ms; x {B * T} images); its first image equals the device's bits: {same}")
    del frames, exact
    torch.cuda.empty_cache()
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
