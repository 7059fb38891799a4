#!/usr/bin/env python3
"""Throughput of the image-forgery evidence (ultrafnd_git_amd/video.py: DeepForgeryDetector.ela_lbp_batch, FaceWarpAnalyzer.score_batch,
forgery_features) on one MI355X: one process, one GPU, unprofiled, uint8 frames resident on the device.

    forgery_throughput.py [--out profiles/forgery_throughput.txt]
        B = 32 clips of 3 frames at 256 x 256 (the resize is the identity) and at 720 x 1280 (downsampling: gather reads); one frame per
        clip is read.  ms per call and images/s of the two class calls and of forgery_features (one resize, one round trip, both
        outputs), with and without the ELA-map output; per stage the time of that stage's launches alone, and the bytes the algorithm
        reads + writes over that time as a share of the HBM peak the project's documents use (8.0 TB/s).
    forgery_throughput.py --cpu
        on a CPU-only host: Pillow's libjpeg encode + decode and the NumPy statistics (the mirror's vectorised forms, not the reference's
        Python loops) one image per call, which is the reference's call pattern; wall clock.

Device events around windows of >= 0.5 s after warm-up, three windows per path, the paths alternated; median.  Run it under a `timeout`.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np

HBM_PEAK = 8.0e12
SHAPES = ((32, 3, 256, 256), (32, 3, 720, 1280))
PLANE = 65536
# integer operations of the DCT stage per 8 x 8 block, a hand ESTIMATE from csrc/forgery.hip (colour conversion, downsample and upsample are not in it): an 8-point LL&M pass is 12 multiplications and 32
# additions / shifts (44), a block runs 8 lines x 4 passes of them, and 64 quantise + dequantise steps of about 8 operations around one
# integer division (counted as 20): 32 x 44 + 64 x 28.  1536 blocks per image (1024 Y, 256 Cb, 256 Cr).
DCT_OPS_PER_IMAGE = 1536 * (32 * 44 + 64 * 28)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--cpu", action="store_true")
a = ap.parse_args()
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def finish():
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(out) + "\n")


if a.cpu:
    import io

    import PIL
    from PIL import Image

    def cpu_image(rgb):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="JPEG", quality=85, subsampling=2)
        buf.seek(0)
        rec = np.asarray(Image.open(buf).convert("RGB"))
        t1 = time.perf_counter()
        ela = np.abs(rgb.astype(np.float32) - rec.astype(np.float32)).astype(np.uint8)
        stats = np.array([ela.mean(), ela.std(), ela.max(), ela.min()], dtype=np.float32)
        gray = (0.2989 * ela[..., 0] + 0.587 * ela[..., 1] + 0.114 * ela[..., 2]).astype(np.uint8).astype(np.int32)
        c, code = gray[1:254:2, 1:254:2], 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    code = code + (gray[1 + dy:254 + dy:2, 1 + dx:254 + dx:2] > c)
        hist = np.bincount(code.ravel(), minlength=10) / 16129.0
        g = (0.2989 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]).astype(np.uint8).astype(np.float32)
        gx, gy = np.zeros_like(g), np.zeros_like(g)
        gx[:, 1:], gy[1:, :] = g[:, 1:] - g[:, :-1], g[1:, :] - g[:-1, :]
        mag = np.sqrt(gx * gx + gy * gy)
        return t1, stats, hist, mag.mean(), mag.std()

    say(f"# Pillow {PIL.__version__} (libjpeg) round trip + NumPy {np.__version__} statistics on this host's CPU, one 256 x 256 image per call, wall clock, "
        "median of 50 calls after 5; the image already resized (the reference's resize is a Python loop of 65,536 iterations on top)")
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    trip, rest = [], []
    for i in range(55):
        t0 = time.perf_counter()
        t1 = cpu_image(img)[0]
        t2 = time.perf_counter()
        if i >= 5:
            trip.append(t1 - t0)
            rest.append(t2 - t1)
    mt, mr = statistics.median(trip) * 1e3, statistics.median(rest) * 1e3
    say(f"CPU per image: JPEG round trip {mt:.3f} ms + statistics {mr:.3f} ms = {mt + mr:.3f} ms = {1e3 / (mt + mr):.0f} images/s; a batch of 32: {32 * (mt + mr):.1f} ms")
    finish()
    raise SystemExit(0)

import torch

from ultrafnd_git_amd import video

if not torch.cuda.is_available():
    raise SystemExit("forgery_throughput.py: no HIP device (timings are taken on the GPU only)")
DEV = torch.device("cuda")


def timed(fn, window_s):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(2, int(window_s / max(time.perf_counter() - t0, 1e-5)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


prop = torch.cuda.get_device_properties(0)
say(f"# tools/forgery_throughput.py on one {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}: uint8 HWC clips resident on the device; "
    f"device events over windows of >= {a.window} s after warm-up, three windows per path (alternated), median; unprofiled.")
say("# detector = DeepForgeryDetector(256).ela_lbp_batch, warp = FaceWarpAnalyzer().score_batch (each its own resize and round trip); one pass = "
    "video.forgery_features (both outputs from one resize and one round trip; + map: the ELA map (B, 256, 256, 3) stored too).  Stage rows: that stage's "
    "launches alone, back to back, so launch gaps are inside; bytes = what the algorithm reads + writes per image (resize 3 + 3 per pixel; dct: rgb in, "
    f"Y + Cb + Cr planes out; upsample: planes in, rgb out; maps: rgb + rec in), share of {HBM_PEAK / 1e12:.1f} TB/s.")
det, warp = video.DeepForgeryDetector(256), video.FaceWarpAnalyzer()
with torch.no_grad():
    for B, T, H, W in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(B * T + H)
        clips = torch.randint(0, 256, (B, T, H, W, 3), dtype=torch.uint8, generator=g).to(DEV)
        st = video.ForgeryStages(clips)
        st.resize(); st.roundtrip(85, 1, 0); st.maps(1.0, 0, lbp=True, grad=True); st.finish(256, grad=True)
        legs = [("detector", lambda: det.ela_lbp_batch(clips)), ("warp", lambda: warp.score_batch(clips)), ("one pass", lambda: video.forgery_features(clips)),
                ("one pass + map", lambda: video.forgery_features(clips, ela_map=True)), ("stage resize", st.resize),
                ("stage roundtrip (dct + upsample)", lambda: st.roundtrip(85, 1, 0)), ("stage roundtrip none (copy)", lambda: st.roundtrip(85, 0, 1)),
                ("stage maps", lambda: st.maps(1.0, 0, lbp=True, grad=True)), ("stage maps + map", lambda: st.maps(1.0, 0, lbp=True, grad=True, ela_map=True)),
                ("stage finish", lambda: st.finish(256, grad=True))]
        rgb, planes = 3 * PLANE, PLANE + PLANE // 2
        nbytes = {"stage resize": B * 2 * rgb, "stage roundtrip (dct + upsample)": B * 2 * (rgb + planes), "stage roundtrip none (copy)": B * 2 * rgb,
                  "stage maps": B * 2 * rgb, "stage maps + map": B * 3 * rgb}
        nbytes["one pass"] = nbytes["stage resize"] + nbytes["stage roundtrip (dct + upsample)"] + nbytes["stage maps"]
        nbytes["one pass + map"] = nbytes["one pass"] + B * rgb
        res = {nm: [] for nm, _ in legs}
        for _ in range(3):
            for nm, fn in legs:
                res[nm].append(timed(fn, a.window))
        med = {}
        for nm, _ in legs:
            ms = [m for m, _ in res[nm]]
            med[nm] = statistics.median(ms)
            rate = f"; {nbytes[nm] / 1e6:.1f} MB -> {nbytes[nm] / med[nm] / 1e9:.3f} TB/s = {nbytes[nm] / med[nm] * 1e3 / HBM_PEAK:.4f} of the HBM peak" if nm in nbytes else ""
            per = f" = {B / med[nm] * 1e3:9.0f} images/s" if not nm.startswith("stage") else ""
            say(f"  B={B} {H}x{W} {nm:34s} {med[nm]:8.4f} ms per call{per} (three windows: {', '.join(f'{m:.4f}' for m in ms)}; "
                f"{res[nm][0][1]} calls per window){rate}")
        stages = {nm: med[nm] for nm in ("stage resize", "stage roundtrip (dct + upsample)", "stage maps", "stage finish")}
        top = max(stages, key=stages.get)
        say(f"  B={B} {H}x{W}: the stage whose time dominates the one-pass call: {top} ({stages[top]:.4f} of {sum(stages.values()):.4f} ms of stage time; "
            f"the call itself {med['one pass']:.4f} ms)")
        ops = B * DCT_OPS_PER_IMAGE
        say(f"  B={B} {H}x{W}: the round trip runs about {ops / 1e6:.0f} M integer operations (a hand estimate of the DCT, quantiser and inverse DCT only: {DCT_OPS_PER_IMAGE} per image) in "
            f"{med['stage roundtrip (dct + upsample)']:.4f} ms = {ops / med['stage roundtrip (dct + upsample)'] / 1e9:.3f} Tops/s over both of its launches, an estimate likewise")
        del clips, st
        torch.cuda.empty_cache()
finish()
