#!/usr/bin/env python3
"""Mint tests/golden/motion.npz from the REAL reference's OpticalFlow3DCNN (src/core_blocks/visual_blocks.py) and ChronosGuard
(src/models/chronos_guard.py).

Needs a checkout of the reference project (it is not part of this repository and never travels with it):

    python tests/golden/make_golden_motion.py <path to the reference checkout>

`cv2` and `skimage` are masked before the import, so both modules take the branches they take on a host without OpenCV (asserted:
_HAS_CV2 and _HAS_SKIMAGE are false wherever they exist).  Each module's `np` is replaced by a pass-through that records the float32
arrays the classes build from Python lists: ChronosGuard's two per-pair series and its seven statistics, OpticalFlow3DCNN's 77 pooled
values.  Seeded uint8 clips with small sources go through extract_features, temporal_tamper_score and extract (dim 256 and 512), and
the clips and every returned or recorded number are stored.  Data only.  About a minute: the reference's resize is a Python loop of
65,536 iterations per frame.

The clips: per-frame gains keep both per-pair series at a coefficient of variation >= 0.05 (asserted; tests/motion_ref.py's bounds for
the reference's float32 statistics rest on it), the static clip and the degenerate short ones excepted.
"""
from __future__ import annotations

import os
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SEED = 2026


class _Tap:
    """numpy, with asarray(list, dtype=float32) recorded."""

    def __init__(self, real):
        self._real, self.seen = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def asarray(self, a, *args, **kw):
        out = self._real.asarray(a, *args, **kw)
        if isinstance(a, list) and kw.get("dtype") is self._real.float32:
            self.seen.append(out.copy())
        return out


def clips(rng):
    """name -> (T, H, W, 3) uint8."""
    def scene(T, H, W, gains, noise=6.0, base=None):
        base = rng.integers(0, 256, (H, W, 3)).astype(np.float64) if base is None else base
        out = [np.clip(base * g + rng.normal(0.0, noise, base.shape), 0, 255).astype(np.uint8) for g in gains[:T]]
        return np.stack(out)

    g = lambda T: rng.uniform(0.35, 1.0, T)
    c = {}
    c["rand7"] = scene(7, 40, 48, g(7))
    blocks = rng.integers(0, 256, (75, 125, 3)).astype(np.float64)       # 300 x 500 from 4 x 4 blocks: the file stays small
    small = scene(5, 75, 125, g(5), noise=10.0, base=blocks)
    c["down5"] = np.repeat(np.repeat(small, 4, axis=1), 4, axis=2)
    c["long12"] = scene(12, 24, 32, g(12))
    c["static6"] = np.repeat(scene(1, 16, 16, [1.0]), 6, axis=0)
    a, b = scene(5, 32, 32, g(5), noise=3.0), scene(4, 32, 32, g(4), noise=3.0)
    c["cut9"] = np.concatenate([a, b])
    ex = scene(6, 32, 32, g(6))
    ex[1] = 0; ex[2] = 0; ex[3] = 255; ex[5] = 255
    c["extremes6"] = ex
    c["four4"] = scene(4, 20, 20, g(4))
    c["three3"] = scene(3, 9, 7, g(3))
    c["two2"] = scene(2, 8, 8, g(2))
    c["nine9"] = scene(9, 12, 10, g(9))
    return c


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "src" / "models" / "chronos_guard.py").is_file():
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.modules["cv2"] = None
    sys.modules["skimage"] = None
    sys.modules["skimage.feature"] = None
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ref))
    import src.core_blocks.visual_blocks as vb
    import src.models.chronos_guard as cg
    for mod in (vb, cg):
        for flag in ("_HAS_CV2", "_HAS_SKIMAGE"):
            assert not getattr(mod, flag, False), (mod.__name__, flag)
    tap_v, tap_c = _Tap(np), _Tap(np)
    vb.np, cg.np = tap_v, tap_c

    rng = np.random.default_rng(SEED)
    store = {"names": []}
    guard, flow256, flow512 = cg.ChronosGuard(feat_dim=128), vb.OpticalFlow3DCNN(dim=256), vb.OpticalFlow3DCNN(dim=512)
    assert not flow256.use_tvl1
    warnings.simplefilter("ignore")
    with np.errstate(all="ignore"):
        for name, clip in clips(rng).items():
            tap_c.seen.clear(); tap_v.seen.clear()
            feats = guard.extract_features(clip)
            cut, flows, stats = tap_c.seen
            score = guard.temporal_tamper_score(clip)
            v256 = flow256.extract(clip)
            v512 = flow512.extract(clip)
            pooled = tap_v.seen[0]
            assert len(tap_v.seen) == 2 and np.array_equal(pooled, tap_v.seen[1], equal_nan=True) and pooled.shape == (77,) and stats.shape == (7,)
            if name not in ("static6", "two2", "three3", "four4"):
                for s in (cut, flows):
                    assert s.std() / s.mean() >= 0.05, (name, s)
            store["names"].append(name)
            for key, val in (("frames", clip), ("cut_scores", cut), ("flows", flows), ("stats", stats), ("features", feats), ("tamper", np.float64(score)),
                             ("pooled", pooled), ("flow256", v256), ("flow512", v512)):
                store[f"{name}/{key}"] = val
            print(name, clip.shape, "tamper", score, "nan:", bool(np.isnan(feats).any()), bool(np.isnan(v256).any()), flush=True)
    assert np.isnan(store["four4/flow256"]).all() and np.isnan(store["static6/features"]).all() and np.isfinite(store["static6/tamper"])
    assert np.isfinite(store["rand7/flow256"]).all() and np.isfinite(store["down5/flow512"]).all()
    store["names"] = np.array(store["names"])
    path = HERE / "motion.npz"
    np.savez_compressed(path, **store)
    assert path.stat().st_size < 1_000_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
