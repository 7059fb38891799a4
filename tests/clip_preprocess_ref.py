"""NumPy restatement of the CLIP image preprocessing the package runs on the device (csrc/clip_preprocess.hip): Pillow's two-pass
fixed-point bicubic resize (horizontal, then vertical, a uint8 image between them), transformers' shortest-edge size rule, the
centre crop and the rescale / normalise value map of the checkpoint's CLIPImageProcessor (its Pillow backend).  It is written from
Pillow's and transformers' documented behaviour, independently of the product's table builder (video.clip_resize_tables): the
product builds only the rows and columns the crop needs, this file resizes the WHOLE image and crops afterwards.

Every step can be done wrong on purpose (`mistakes`, a set of names from MISTAKES): the tests show that each named mistake
changes an output, so the equalities they assert are not vacuous.
"""
from __future__ import annotations

import hashlib
import math
from pathlib import Path

import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
RESCALE = 0.00392156862745098       # the processor's rescale_factor, 1 / 255 as a double
BITS = 22                           # fractional bits of Pillow's coefficients

MISTAKES = ("no_antialias", "a_075", "round_negative_up", "vertical_first", "float_intermediate", "centre_no_half", "long_edge_rounded",
            "crop_round_up", "map_f32_reciprocal_first", "map_double", "map_divide_255_f32")

# the source sizes (H, W) of the issue
SIZES = ((90, 160), (100, 75), (224, 224), (225, 223), (224, 398), (256, 256), (480, 854), (37, 500), (720, 1280), (1080, 1920))
PATTERNS = ("noise", "hramp", "vramp", "binary", "checker", "zeros", "ones")


def pattern(name: str, H: int, W: int, seed: int) -> np.ndarray:
    """(H, W, 3) uint8.  Seeded: noise and binary depend on (seed, H, W) alone."""
    rng = np.random.default_rng([seed, H, W])
    if name == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if name == "binary":
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    if name == "hramp":
        r = (np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)
        return np.stack([np.broadcast_to(r[None, :], (H, W)), np.broadcast_to(r[None, ::-1], (H, W)), np.full((H, W), 128, np.uint8)], -1).copy()
    if name == "vramp":
        r = (np.arange(H) * 255 // max(H - 1, 1)).astype(np.uint8)
        return np.stack([np.broadcast_to(r[:, None], (H, W)), np.full((H, W), 7, np.uint8), np.broadcast_to(r[::-1, None], (H, W))], -1).copy()
    if name == "checker":
        c = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)
        return np.stack([c, 255 - c, c], -1)
    if name == "zeros":
        return np.zeros((H, W, 3), np.uint8)
    if name == "ones":
        return np.full((H, W, 3), 255, np.uint8)
    raise ValueError(name)


def output_size(H: int, W: int, S: int, mistakes=()) -> tuple:
    """(h', w') of the resized image: the short edge becomes S, the long edge int(S * long / short)."""
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(S * long_ / short + 0.5) if "long_edge_rounded" in mistakes else int(S * long_ / short)
    return (new_long, S) if W <= H else (S, new_long)


def _bicubic(t: float, a: float) -> float:
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def coefficients(n_in: int, n_out: int, mistakes=(), fixed: bool = True):
    """One pass of n_in -> n_out samples: (xmin[n_out], count[n_out], k[n_out][ksize]); k int32 with 22 fractional bits, or the
    normalised float64 weights with fixed=False."""
    a = -0.75 if "a_075" in mistakes else -0.5
    scale = n_in / n_out
    fs = 1.0 if "no_antialias" in mistakes else max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    xmin = np.zeros(n_out, np.int64)
    cnt = np.zeros(n_out, np.int64)
    kk = np.zeros((n_out, ksize), np.float64)
    for xx in range(n_out):
        c = xx * scale if "centre_no_half" in mistakes else (xx + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        hi = max(hi, lo)
        n = hi - lo
        ww = 0.0
        for x in range(n):
            w = _bicubic((x + lo - c + 0.5) * ss, a)
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            for x in range(n):
                kk[xx, x] /= ww
        xmin[xx], cnt[xx] = lo, n
    if not fixed:
        return xmin, cnt, kk
    v = kk * float(1 << BITS)
    up = np.trunc(v + 0.5)
    down = up if "round_negative_up" in mistakes else np.trunc(v - 0.5)
    return xmin, cnt, np.where(kk < 0, down, up).astype(np.int32)


def _pass(img: np.ndarray, n_out: int, axis: int, mistakes=()) -> np.ndarray:
    """Resample `axis` (0: rows, 1: columns) of an (h, w, 3) image to n_out samples."""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    floating = "float_intermediate" in mistakes
    xmin, cnt, k = coefficients(n_in, n_out, mistakes, fixed=not floating)
    src = np.moveaxis(img, axis, 0)
    out = np.empty((n_out,) + src.shape[1:], np.float64 if floating else np.uint8)
    for xx in range(n_out):
        seg = src[xmin[xx]:xmin[xx] + cnt[xx]]
        if floating:
            out[xx] = np.tensordot(k[xx, :cnt[xx]], seg.astype(np.float64), axes=(0, 0))
        else:
            acc = np.tensordot(k[xx, :cnt[xx]].astype(np.int64), seg.astype(np.int64), axes=(0, 0)) + (1 << (BITS - 1))
            assert np.abs(acc).max() < 2 ** 31
            out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, S: int = 224, mistakes=()) -> np.ndarray:
    """(H, W, 3) uint8 -> the whole resized image (h', w', 3) uint8."""
    h2, w2 = output_size(img.shape[0], img.shape[1], S, mistakes)
    if "vertical_first" in mistakes:
        out = _pass(_pass(img, h2, 0, mistakes), w2, 1, mistakes)
    else:
        out = _pass(_pass(img, w2, 1, mistakes), h2, 0, mistakes)
    if out.dtype != np.uint8:
        out = np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)
    return out


def crop_offsets(h2: int, w2: int, S: int, mistakes=()) -> tuple:
    if "crop_round_up" in mistakes:
        return (h2 - S + 1) // 2, (w2 - S + 1) // 2
    return (h2 - S) // 2, (w2 - S) // 2


def value_table(mean=CLIP_MEAN, std=CLIP_STD, mistakes=()) -> np.ndarray:
    """(3, 256) float32: what channel c maps byte v to."""
    v = np.arange(256)
    m32, s32 = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    if "map_double" in mistakes:
        return (((v.astype(np.float64) * RESCALE)[None, :] - m32.astype(np.float64)[:, None]) / s32.astype(np.float64)[:, None]).astype(np.float32)
    if "map_f32_reciprocal_first" in mistakes:
        r = v.astype(np.float32) * np.float32(RESCALE)
    elif "map_divide_255_f32" in mistakes:
        r = (v.astype(np.float64) * np.float64(np.float32(1.0) / np.float32(255.0))).astype(np.float32)      # the double product, the reciprocal in fp32
    else:
        r = (v.astype(np.float64) * RESCALE).astype(np.float32)
    return ((r[None, :] - m32[:, None]) / s32[:, None]).astype(np.float32)


def preprocess(img: np.ndarray, S: int = 224, mean=CLIP_MEAN, std=CLIP_STD, mistakes=()):
    """(H, W, 3) uint8 -> (rgb (S, S, 3) uint8, pixel_values (3, S, S) float32)."""
    full = resize(img, S, mistakes)
    top, left = crop_offsets(full.shape[0], full.shape[1], S, mistakes)
    rgb = np.ascontiguousarray(full[top:top + S, left:left + S])
    lut = value_table(mean, std, mistakes)
    pv = np.stack([lut[c][rgb[..., c]] for c in range(3)], 0)
    return rgb, pv


def tables(H: int, W: int, S: int = 224) -> dict:
    """What video.clip_resize_tables must return, from the whole-image coefficients cut to the crop."""
    h2, w2 = output_size(H, W, S)
    top, left = crop_offsets(h2, w2, S)
    out = {"resized": (h2, w2), "top": top, "left": left}
    for name, n_in, n_out, off in (("h", W, w2, left), ("v", H, h2, top)):
        if n_in == n_out:      # a skipped pass is the identity: one tap of weight 1
            first, cnt, k = np.arange(off, off + S), np.ones(S, np.int64), np.full((S, 1), 1 << BITS, np.int32)
        else:
            xmin, c, kk = coefficients(n_in, n_out)
            first, cnt = xmin[off:off + S], c[off:off + S]
            k = kk[off:off + S, :int(cnt.max())]
        out[name] = {"first": first.astype(np.int32), "count": cnt.astype(np.int32), "k": np.ascontiguousarray(k, dtype=np.int32), "skipped": n_in == n_out}
    return out


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_fixture(path: Path) -> dict:
    """tests/golden/clip_preprocess.npz -> {case name: {H, W, S, pattern, seed, rgb_sha, pv_sha, rgb_corner, pv_corner}} and "versions"."""
    z = np.load(path, allow_pickle=False)
    names = [str(n) for n in z["names"]]
    cases = {}
    for i, n in enumerate(names):
        H, W, S, seed = (int(x) for x in z["shapes"][i])
        cases[n] = {"H": H, "W": W, "S": S, "seed": seed, "pattern": str(z["patterns"][i]), "rgb_sha": str(z["rgb_sha"][i]), "pv_sha": str(z["pv_sha"][i]),
                    "rgb_corner": z["rgb_corner"][i], "pv_corner": z["pv_corner"][i]}
    return {"cases": cases, "versions": str(z["versions"])}


def golden_cases() -> tuple:
    """(name, H, W, S, pattern, seed) of every case of tests/golden/clip_preprocess.npz: two frames (noise, 0/255 noise) per size of the
    issue, the other patterns at two sizes, a portrait source whose horizontal pass is skipped, and the output edges 223 and 225."""
    cases = []
    for H, W in SIZES:
        cases += [(H, W, 224, "noise", 1), (H, W, 224, "binary", 2)]
    for H, W in ((100, 75), (480, 854)):
        cases += [(H, W, 224, p, 3) for p in ("hramp", "vramp", "checker", "zeros", "ones")]
    cases += [(398, 224, 224, "noise", 1), (398, 224, 224, "binary", 2)]
    for S in (223, 225):
        cases += [(100, 75, S, "noise", 1), (90, 160, S, "binary", 2)]
    return tuple((f"{H}x{W}_s{S}_{p}{seed}", H, W, S, p, seed) for H, W, S, p, seed in cases)


def case_name(H: int, W: int, S: int, pat: str, seed: int) -> str:
    return f"{H}x{W}_s{S}_{pat}{seed}"
