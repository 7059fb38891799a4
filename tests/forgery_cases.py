"""TEST INFRASTRUCTURE: the cases of the image-forgery tests (tests/test_forgery_ref.py, tests/test_gpu_forgery.py) and of the fixture
tests/golden/forgery.npz (tests/golden/make_golden_forgery.py mints it from the reference's own classes).

  CLIPS      small source clips (T, H, W, 3) uint8 that the fixture stores with the reference's vectors and scores; the middle frame of each
             is what both classes read
  SETTINGS   the detector settings the fixture holds per clip: "none" is the reference as it runs without OpenCV (rec = rgb), the others
             the reference with its JPEG re-encode done by Pillow's libjpeg at (quality, scale)
  PLANES     the clips whose Pillow-decoded 256 x 256 image the fixture stores, and at which quality
  full_images   256 x 256 images built at test time (nothing is stored): content at pixel pitch, where the DCT, the range limit, the
             downsampler's alternating bias and the upsampler's edge rules can go wrong
"""
from __future__ import annotations

from typing import Dict

import numpy as np

SEED = 2027
SETTINGS = {"none": None, "q85s1": (85, 1.0), "q50s05": (50, 0.5), "q1s10": (1, 10.0), "q100s1": (100, 1.0)}
PLANES = {"noise5": 85, "sat1": 1, "ramp3": 100}
DIMS = (256, 10)                       # tiled (14 values into 256) and cut (the first 10 of the 14)


def clips() -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(SEED)
    c = {}
    c["noise5"] = rng.integers(0, 256, (5, 40, 48, 3), dtype=np.uint8)                        # middle frame 2
    yy, xx = np.mgrid[0:32, 0:32]
    ramp = np.stack([8 * xx, 8 * yy, 4 * (xx + yy)], axis=-1).astype(np.float64)
    c["ramp3"] = np.stack([np.clip(ramp + rng.normal(0, s, ramp.shape), 0, 255).astype(np.uint8) for s in (9.0, 2.0, 5.0)])      # frame 1
    c["sat1"] = (rng.integers(0, 2, (1, 24, 24, 3)) * 255).astype(np.uint8)                   # 0 / 255 only
    c["flat2"] = rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8)                         # 16 x 16 source: flat 16 x 16 blocks, AC all zero
    c["static2"] = np.full((2, 8, 8, 3), (90, 160, 30), dtype=np.uint8)                       # one colour: g_mean = 0
    c["wide2"] = rng.integers(0, 256, (2, 20, 300, 3), dtype=np.uint8)                        # wider than 256: sampled pixels are strided
    c["one1"] = np.array([[[[200, 17, 99]]]], dtype=np.uint8)                                 # a 1 x 1 source
    return c


def full_images() -> Dict[str, np.ndarray]:
    """name -> (256, 256, 3) uint8."""
    rng = np.random.default_rng(SEED + 1)
    yy, xx = np.mgrid[0:256, 0:256]
    im = {}
    im["noise"] = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    im["ramp"] = np.stack([xx, yy, (xx + yy) // 2], axis=-1).astype(np.uint8)
    im["saturated"] = (rng.integers(0, 2, (256, 256, 3)) * 255).astype(np.uint8)              # the IDCT overshoots: range limit
    im["blocks"] = np.repeat(np.repeat(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), 16, axis=0), 16, axis=1)
    im["checker"] = np.stack([((xx + yy) & 1) * 255, (xx & 1) * 200 + 20, (yy & 1) * 255], axis=-1).astype(np.uint8)      # period 2
    edges = np.full((256, 256, 3), 128, dtype=np.uint8)                                       # extremes in rows / columns 0 and 255
    edges[0], edges[255], edges[:, 0], edges[:, 255] = (255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 0)
    edges[0, 0], edges[255, 255], edges[0, 255], edges[255, 0] = (0, 0, 0), (255, 255, 255), (255, 0, 255), (0, 255, 255)
    im["edges"] = edges
    return im
