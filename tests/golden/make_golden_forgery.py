#!/usr/bin/env python3
"""Mint tests/golden/forgery.npz from the REAL reference's DeepForgeryDetector and FaceWarpAnalyzer (src/core_blocks/visual_blocks.py).

Needs a checkout of the reference project (it is not part of this repository and never travels with it) and Pillow:

    python tests/golden/make_golden_forgery.py <path to the reference checkout>

`cv2` and `skimage` are masked before the import, so the module takes the branches it takes on a host without OpenCV and scikit-image
(asserted).  Two sets are minted over the clips of tests/forgery_cases.py:

  none     the classes as they run: _jpeg_reencode returns a copy, the ELA map is zero, the LBP histogram that of a zero plane, the score
           its gradient half
  q..s..   DeepForgeryDetector._jpeg_reencode replaced, in this script, by a JPEG encode and decode through Pillow's libjpeg at the
           detector's ela_quality (baseline, 4:2:0: what cv2.imencode(".jpg") writes); every other line of the reference runs as written

Stored: the clips, per setting the vectors at dim 256 and 10, the scores, and for three clips the 256 x 256 image Pillow decoded.  Data only.
"""
from __future__ import annotations

import io
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import forgery_cases as cases  # noqa: E402


def pillow_reencode(self, rgb: np.ndarray) -> np.ndarray:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=self.ela_quality, subsampling=2, optimize=False, progressive=False)
    buf.seek(0)
    dec = np.asarray(Image.open(buf).convert("RGB")).copy()
    pillow_reencode.last = dec
    return dec


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "src" / "core_blocks" / "visual_blocks.py").is_file():
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.modules["cv2"] = None
    sys.modules["skimage"] = None
    sys.modules["skimage.feature"] = None
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ref))
    import src.core_blocks.visual_blocks as vb
    assert not vb._HAS_CV2 and not vb._HAS_SKIMAGE
    original = vb.DeepForgeryDetector._jpeg_reencode

    store = {"names": []}
    for name, clip in cases.clips().items():
        store["names"].append(name)
        store[f"{name}/frames"] = clip
        for setting, qs in cases.SETTINGS.items():
            vb.DeepForgeryDetector._jpeg_reencode = original if qs is None else pillow_reencode
            kw = {} if qs is None else dict(ela_quality=qs[0], ela_scale=qs[1])
            for dim in cases.DIMS:
                v = vb.DeepForgeryDetector(dim=dim, **kw).ela_lbp(clip)
                assert v.dtype == np.float32 and v.shape == (dim,)
                store[f"{name}/{setting}/vec{dim}"] = v
            if qs is not None and cases.PLANES.get(name) == qs[0]:
                store[f"{name}/rec{qs[0]}"] = pillow_reencode.last
            if setting in ("none", "q85s1"):      # the score's detector is always DeepForgeryDetector(dim=16): quality 85, scale 1
                store[f"{name}/{setting}/score"] = np.float64(vb.FaceWarpAnalyzer().score(clip))
            print(name, setting, store[f"{name}/{setting}/vec256"][:4], store.get(f"{name}/{setting}/score"), flush=True)
    vb.DeepForgeryDetector._jpeg_reencode = original
    assert sum(k.split("/")[-1].startswith("rec") for k in store) == len(cases.PLANES)
    store["names"] = np.array(store["names"])
    path = HERE / "forgery.npz"
    np.savez_compressed(path, **store)
    assert path.stat().st_size < 1_000_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
