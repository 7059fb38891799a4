#!/usr/bin/env python3
"""Throughput of the video motion forensics (ultrafnd_git_amd/video.py: ChronosGuard.analyze_batch + OpticalFlow3DCNN.extract_batch) on one
MI355X: one process, one GPU, unprofiled, uint8 clips resident on the device.

    motion_throughput.py [--out profiles/motion_throughput.txt]
        B = 32 x 30 frames of 256 x 256 (the resize is the identity, rows contiguous) and B = 32 x 8 frames of 720 x 1280 (downsampling:
        gather reads): ms per call and clips/s of the two class calls (each runs its own gray pass and walk through time) and of
        motion_features (one gray pass, one walk, both finishes); per stage the time of that stage's launch alone, and the bytes the
        algorithm reads + writes over that time as a share of the HBM peak the project's documents use (8.0 TB/s).
    motion_throughput.py --reference DIR
        on a CPU-only host: the reference's own two classes (DIR: a checkout of the reference) on ONE clip of 3 frames per size, wall
        clock, extrapolated linearly in the pair count to the batches above (the reference's cost is two Python resize loops per pair
        and class, so it is linear in the pairs).

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
SHAPES = ((32, 30, 256, 256), (32, 8, 720, 1280))
PLANE = 65536

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--window", type=float, default=0.5)
ap.add_argument("--reference", default=None)
a = ap.parse_args()
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def finish():
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(out) + "\n")


if a.reference:
    sys.modules["cv2"] = None
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(Path(a.reference).resolve()))
    import warnings

    import src.core_blocks.visual_blocks as vb
    import src.models.chronos_guard as cg
    assert not vb._HAS_CV2 and not cg._HAS_CV2
    warnings.simplefilter("ignore")
    say(f"# the reference's ChronosGuard.extract_features + OpticalFlow3DCNN.extract on this host's CPU (NumPy {np.__version__}, no OpenCV), ONE clip of 3 "
        "frames (2 pairs) per size, wall clock; extrapolated linearly in the pair count")
    rng = np.random.default_rng(0)
    for B, T, H, W in SHAPES:
        clip = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        with np.errstate(all="ignore"):
            t0 = time.perf_counter()
            cg.ChronosGuard().extract_features(clip)
            t1 = time.perf_counter()
            vb.OpticalFlow3DCNN().extract(clip)
            t2 = time.perf_counter()
        per_pair = (t2 - t0) / 2
        say(f"reference CPU {H}x{W}: extract_features {t1 - t0:.2f} s, extract {t2 - t1:.2f} s for 2 pairs = {per_pair:.2f} s per pair -> extrapolated "
            f"{per_pair * (T - 1):.1f} s per clip of {T} frames, {per_pair * (T - 1) * B:.0f} s per batch of {B}")
    finish()
    raise SystemExit(0)

import torch

from ultrafnd_git_amd import video

if not torch.cuda.is_available():
    raise SystemExit("motion_throughput.py: no HIP device (timings are taken on the GPU only)")
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
say(f"# tools/motion_throughput.py on one {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}: uint8 HWC clips resident on the device; "
    f"device events over windows of >= {a.window} s after warm-up, three windows per path (alternated), median; unprofiled.")
say("# classes = ChronosGuard(128).analyze_batch + OpticalFlow3DCNN(256).extract_batch (two gray passes, two walks); one pass = video.motion_features (the same "
    "outputs from one gray pass and one walk).  Stage rows: that stage's launch alone, back to back, so launch gaps are inside; bytes = what the algorithm "
    f"reads + writes (gray: 3 sampled source bytes in and 1 byte out per output pixel; pairs: every gray plane once), share of {HBM_PEAK / 1e12:.1f} TB/s.")
guard, flow = video.ChronosGuard(128), video.OpticalFlow3DCNN(256)
gray_rate = {}
with torch.no_grad():
    for B, T, H, W in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(B * T + H)
        clips = torch.randint(0, 256, (B, T, H, W, 3), dtype=torch.uint8, generator=g).to(DEV)
        st = video.MotionStages(clips)
        st.gray(); st.pairs(True, 3); st.chronos(128); st.flow(256)
        legs = [("classes", lambda: (guard.analyze_batch(clips), flow.extract_batch(clips))), ("one pass", lambda: video.motion_features(clips)),
                ("stage gray", st.gray), ("stage pairs+pyramid", lambda: st.pairs(True, 3)), ("stage pairs only", lambda: st.pairs(True, 0)),
                ("stage chronos finish", lambda: st.chronos(128)), ("stage flow finish", lambda: st.flow(256))]
        frames = B * T
        nbytes = {"stage gray": frames * PLANE * 4 + frames * 16 * 32 * 4, "stage pairs+pyramid": frames * PLANE, "stage pairs only": frames * PLANE}
        nbytes["one pass"] = nbytes["stage gray"] + nbytes["stage pairs+pyramid"]
        nbytes["classes"] = 2 * nbytes["stage gray"] + 2 * frames * PLANE
        res = {nm: [] for nm, _ in legs}
        for _ in range(3):
            for nm, fn in legs:
                res[nm].append(timed(fn, a.window))
        med = {}
        for nm, _ in legs:
            ms = [m for m, _ in res[nm]]
            med[nm] = statistics.median(ms)
            rate = f"; {nbytes[nm] / 1e6:.1f} MB -> {nbytes[nm] / med[nm] / 1e9:.3f} TB/s = {nbytes[nm] / med[nm] * 1e3 / HBM_PEAK:.3f} of the HBM peak" if nm in nbytes else ""
            per = f" = {B / med[nm] * 1e3:9.0f} clips/s" if not nm.startswith("stage") else ""
            say(f"  B={B} T={T} {H}x{W} {nm:22s} {med[nm]:8.3f} ms per call{per} (three windows: {', '.join(f'{m:.3f}' for m in ms)}; "
                f"{res[nm][0][1]} calls per window){rate}")
        stages = {nm: med[nm] for nm in ("stage gray", "stage pairs+pyramid", "stage chronos finish", "stage flow finish")}
        top = max(stages, key=stages.get)
        say(f"  B={B} T={T} {H}x{W}: the stage whose time dominates the one-pass call: {top} ({stages[top]:.3f} of {sum(stages.values()):.3f} ms of stage time; "
            f"the call itself {med['one pass']:.3f} ms)")
        gray_rate[(H, W)] = frames / med["stage gray"] * 1e3
        del clips, st
        torch.cuda.empty_cache()
(h0, w0), (h1, w1) = SHAPES[0][2:], SHAPES[1][2:]
say(f"# gray: {gray_rate[(h0, w0)]:.0f} frames/s at {h0}x{w0} (identity, a frame's sampled bytes are contiguous) against {gray_rate[(h1, w1)]:.0f} frames/s at "
    f"{h1}x{w1} (ratio {gray_rate[(h1, w1)] / gray_rate[(h0, w0)]:.2f}): at {h1}x{w1} the sampled pixels lie {w1 // 256} pixels = {3 * (w1 // 256)} bytes apart, "
    f"so every 128-byte line of a sampled row is fetched for {128 // (3 * (w1 // 256)) * 3} useful bytes -- {256 * w1 * 3 / 1e3:.0f} kB of lines per frame for "
    f"{PLANE * 3 / 1e3:.0f} kB used -- through byte loads no two of which share a dword; the share of the HBM peak above counts the useful bytes only.")
finish()
