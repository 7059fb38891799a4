#!/usr/bin/env python3
"""Measured differences of the CLIP image preprocessing (ultrafnd_git_amd/video.py: clip_preprocess, csrc/clip_preprocess.hip) from the
NumPy restatement tests/clip_preprocess_ref.py and from the fixture minted from Pillow and CLIPImageProcessorPil.

    clip_preprocess_errors.py [--out profiles/clip_preprocess_errors.txt]
        per case of tests/golden/clip_preprocess.npz, in both layouts: the number of rgb bytes and of pixel_values float32 bit patterns
        that differ from the restatement (0 expected), and whether the SHA-256 of each equals the fixture's;
        then, on the host alone, how many outputs each named mistake of the restatement changes (480 x 854 and 37 x 500 noise).
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np
import torch

import clip_preprocess_ref as R
from ultrafnd_git_amd import video

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("clip_preprocess_errors.py measures the kernel on a GPU: none found (no CPU fallback)")
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
fx = R.load_fixture(REPO / "tests" / "golden" / "clip_preprocess.npz")
say(f"# clip_preprocess on {torch.cuda.get_device_name(0)} against tests/clip_preprocess_ref.py and the fixture ({fx['versions']})")
say(f"{'case':28s} {'taps h/v':>9s} {'tile':>5s} {'rows':>5s} {'rgb != (HWC/CHW)':>17s} {'values != (HWC/CHW)':>20s} {'fixture hashes':>15s}")
total = 0
for name, H, W, S, pat, seed in R.golden_cases():
    img = R.pattern(pat, H, W, seed)
    rgb, pv = R.preprocess(img, S)
    t = video.clip_resize_tables(H, W, S)
    hwc = torch.from_numpy(img)[None, None].cuda()
    d = []
    ok = True
    for frames, lay in ((hwc, "HWC"), (hwc.permute(0, 1, 4, 2, 3).contiguous(), "CHW")):
        got = {k: v.cpu().numpy()[0, 0] for k, v in video.clip_preprocess(frames, layout=lay, image_size=S, want=("pixel_values", "rgb")).items()}
        d.append((int((got["rgb"] != rgb).sum()), int((bits(got["pixel_values"]) != bits(pv)).sum())))
        ok &= R.sha(got["rgb"]) == fx["cases"][name]["rgb_sha"] and R.sha(got["pixel_values"]) == fx["cases"][name]["pv_sha"]
    total += sum(x + y for x, y in d)
    say(f"{name:28s} {t['h']['k'].shape[1]:4d}/{t['v']['k'].shape[1]:<4d} {t['tile_rows']:5d} {t['lds_rows']:5d} {d[0][0]:8d}/{d[1][0]:<8d} {d[0][1]:9d}/{d[1][1]:<10d} "
        f"{'equal' if ok else 'DIFFER':>15s}")
say(f"# differing bytes and values over all cases and layouts: {total}")
say("# the restatement's named mistakes, host only: outputs changed (rgb bytes / pixel_values bit patterns) of 150528 each")
for m in R.MISTAKES:
    row = []
    for H, W in ((480, 854), (37, 500)):
        img = R.pattern("noise", H, W, 5)
        rgb, pv = R.preprocess(img)
        rgb2, pv2 = R.preprocess(img, mistakes=(m,))
        row.append(f"{H}x{W}: {int((rgb2 != rgb).sum()):6d} / {int((bits(pv2) != bits(pv)).sum()):6d}")
    say(f"  {m:26s} " + "    ".join(row))
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
