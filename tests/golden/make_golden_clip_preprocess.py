#!/usr/bin/env python3
"""Mint tests/golden/clip_preprocess.npz from Pillow and transformers' CLIPImageProcessorPil (the image processor the reference
instantiates for its CLIP checkpoint, on its Pillow backend):

    python tests/golden/make_golden_clip_preprocess.py

Per case of tests/clip_preprocess_ref.golden_cases(): the generator's pattern, seed and shape (the frame is rebuilt from them, it is
not stored), the SHA-256 of the cropped resized image's bytes (PIL.Image.resize(BICUBIC), cropped) and of the processor's
pixel_values bytes, and the top-left 16 x 16 x 3 corner of each.  The library versions are recorded.  Data only; the GPU test needs
neither library.  The generator asserts that the NumPy restatement equals both in every byte and bit.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def main():
    sys.path.insert(0, str(HERE.parent))
    import PIL
    import transformers
    from PIL import Image
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    import clip_preprocess_ref as R

    store = {k: [] for k in ("names", "shapes", "patterns", "rgb_sha", "pv_sha", "rgb_corner", "pv_corner")}
    for name, H, W, S, pat, seed in R.golden_cases():
        img = R.pattern(pat, H, W, seed)
        proc = CLIPImageProcessorPil(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
        pv = np.ascontiguousarray(proc(images=Image.fromarray(img), return_tensors="np")["pixel_values"][0])
        h2, w2 = R.output_size(H, W, S)
        full = np.asarray(Image.fromarray(img).resize((w2, h2), Image.BICUBIC))
        top, left = R.crop_offsets(h2, w2, S)
        rgb = np.ascontiguousarray(full[top:top + S, left:left + S])
        assert pv.dtype == np.float32 and pv.shape == (3, S, S) and rgb.shape == (S, S, 3)
        mine_rgb, mine_pv = R.preprocess(img, S)
        assert np.array_equal(mine_rgb, rgb) and np.array_equal(mine_pv.view(np.uint32), pv.view(np.uint32)), name
        store["names"].append(name)
        store["shapes"].append((H, W, S, seed))
        store["patterns"].append(pat)
        store["rgb_sha"].append(R.sha(rgb))
        store["pv_sha"].append(R.sha(pv))
        store["rgb_corner"].append(rgb[:16, :16].copy())
        store["pv_corner"].append(pv[:, :16, :16].copy())
        print(f"{name:28s} rgb {store['rgb_sha'][-1][:12]} pixel_values {store['pv_sha'][-1][:12]}", flush=True)
    out = {"names": np.array(store["names"]), "shapes": np.array(store["shapes"], np.int64), "patterns": np.array(store["patterns"]),
           "rgb_sha": np.array(store["rgb_sha"]), "pv_sha": np.array(store["pv_sha"]), "rgb_corner": np.stack(store["rgb_corner"]),
           "pv_corner": np.stack(store["pv_corner"]),
           "versions": np.array(f"Pillow {PIL.__version__}, transformers {transformers.__version__} (CLIPImageProcessorPil), numpy {np.__version__}")}
    path = HERE / "clip_preprocess.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < 400_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes;", str(out["versions"]))


if __name__ == "__main__":
    main()
