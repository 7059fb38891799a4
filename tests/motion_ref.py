"""TEST INFRASTRUCTURE for ultrafnd_git_amd/video.py (CPU, NumPy): a vectorised mirror of the reference's OpenCV-less branches of
OpticalFlow3DCNN (src/core_blocks/visual_blocks.py) and ChronosGuard (src/models/chronos_guard.py), and the bounds of its float parts.

Exact quantities (integers, or float32 values that are exact by construction):
  to_uint8          the per-frame float -> uint8 rule
  source_index      nearest neighbour: output y reads source row (y H) >> 8 (= floor(y H / 256))
  luma / gray       (0.2989 r + 0.587 g + 0.114 b) in float64, truncated: (T, 256, 256) uint8
  HIST_LUT, hist32  np.histogram(bins=32, range=(0, 255)) of a uint8 plane is a table lookup: min(31, 32 v // 255)
  pair_sums, flow_mags   sum |d| per pair as integers; / 65536 in float32 is exact (every partial sum is an integer < 2^24)
  chunks            the 1-2-4 temporal pyramid's (lo, hi) pair ranges, as array slicing clips them
  chunk_planes      m = fl32(sum |d|) / fl32(n), a = fl32(0.25 (2n + sum sign d)) / fl32(n): with the frame-difference flow a pair's angle
                    is exactly 0.75, 0.25 or 0.5 (d > 0, < 0, = 0), so the sums are exact in any order and two float32 divisions remain
  bins8             np.histogram(bins=8, range=(0, 1)) of float32 a: min(7, floor(8 a))
float64 evaluations (the yardstick for everything the reference accumulates in float32):
  cut_scores64, chronos_stats64, pooled64, tile_normalise64, tamper64
Bounds for a float32 evaluation of those against float64 (u = 2^-24, derivations beside each): mean_bound, std_bound, corr_bound,
vector_bound.  They bound the reference's own NumPy float32 arithmetic (tests/test_motion_ref.py holds the fixture to them), so no
bound is tighter than the yardstick; the GPU, which evaluates the statistics in double and rounds once, sits far inside.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np

SIDE, PLANE = 256, 65536
U32 = 2.0 ** -24                      # unit roundoff of float32
BIN_WIDTH = 7.96875                   # 255 / 32, exact
HIST_LUT = np.minimum(31, (32 * np.arange(256)) // 255)
ANGLES = {1: 0.75, -1: 0.25, 0: 0.5}  # (arctan2(d, 0) + pi) / (2 pi) in float32, by the sign of d
CLIP_NAMES_DEGENERATE = ("static6", "two2", "three3", "four4")


# ------------------------------------------------------------------ exact part
def to_uint8(frames: np.ndarray) -> np.ndarray:
    """(T, ...) non-uint8 frames -> uint8 by the per-frame rule: max <= 1 + 1e-6 -> x 255; clip to 0..255; truncate."""
    if frames.dtype == np.uint8:
        return frames
    out = []
    for f in frames:
        f = f * 255.0 if f.max() <= 1.0 + 1e-6 else f
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return np.stack(out)


def source_index(n: int) -> np.ndarray:
    return (np.arange(SIDE, dtype=np.int64) * n) >> 8


def luma(rgb: np.ndarray) -> np.ndarray:
    """(..., 3) uint8 -> (...) uint8: float64 arithmetic in this operation order, then truncation."""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return (0.2989 * r + 0.587 * g + 0.114 * b).astype(np.uint8)


def gray(clip: np.ndarray) -> np.ndarray:
    """(T, H, W, 3) uint8 -> (T, 256, 256) uint8."""
    assert clip.dtype == np.uint8 and clip.ndim == 4 and clip.shape[3] == 3
    iy, ix = source_index(clip.shape[1]), source_index(clip.shape[2])
    return luma(clip[:, iy][:, :, ix])


def hist32(g: np.ndarray) -> np.ndarray:
    """(T, 256, 256) uint8 -> (T, 32) int64 counts."""
    return np.stack([np.bincount(HIST_LUT[p].ravel(), minlength=32) for p in g])


def diffs(g: np.ndarray) -> np.ndarray:
    return g[1:].astype(np.int32) - g[:-1].astype(np.int32)


def pair_sums(g: np.ndarray) -> np.ndarray:
    return np.abs(diffs(g)).reshape(max(len(g) - 1, 0), PLANE).sum(axis=1).astype(np.int64)


def flow_mags(g: np.ndarray) -> np.ndarray:
    return (pair_sums(g).astype(np.float32) / np.float32(PLANE)).astype(np.float32)


def chunks(pairs: int, levels: int = 3) -> List[Tuple[int, int]]:
    out = []
    for level in range(levels):
        parts = 2 ** level
        seg = max(1, pairs // parts)
        for p in range(parts):
            lo, hi = min(p * seg, pairs), (min((p + 1) * seg, pairs) if p < parts - 1 else pairs)
            out.append((lo, max(lo, hi)))
    return out


def chunk_planes(d: np.ndarray, lo: int, hi: int) -> Tuple[np.ndarray, np.ndarray]:
    """The per-pixel mean magnitude and mean angle planes (float32) of pairs [lo, hi); NaN planes for an empty chunk."""
    n = hi - lo
    if n <= 0:
        nan = np.full((SIDE, SIDE), np.nan, np.float32)
        return nan, nan.copy()
    mag = np.abs(d[lo:hi]).sum(axis=0).astype(np.float32)                  # integers < 2^24: exact
    sgn = np.sign(d[lo:hi]).sum(axis=0)
    ang = (np.float32(0.25) * (2 * n + sgn).astype(np.float32)).astype(np.float32)
    return mag / np.float32(n), ang / np.float32(n)


def bins8(a: np.ndarray) -> np.ndarray:
    a = a[~np.isnan(a)]
    return np.bincount(np.minimum(7, np.floor(np.float32(8.0) * a).astype(np.int64)), minlength=8)


# ------------------------------------------------------------------ float64 evaluations
def cut_scores64(h: np.ndarray) -> np.ndarray:
    """(T, 32) counts -> (T - 1,) float64: sum_k |c0_k / w / N - c1_k / w / N|."""
    dens = h.astype(np.float64) / BIN_WIDTH / float(PLANE)
    return np.abs(dens[:-1] - dens[1:]).sum(axis=1)


def chronos_stats64(cut: np.ndarray, flow: np.ndarray) -> np.ndarray:
    """The seven statistics of two per-pair series, in float64 (NaN correlation for a series without variance, as np.corrcoef)."""
    c, f = np.asarray(cut, np.float64), np.asarray(flow, np.float64)
    if c.size == 0:
        return np.zeros(7)
    corr = 0.0
    if c.size > 3:
        dc, df = c - c.mean(), f - f.mean()
        with np.errstate(all="ignore"):
            corr = float(np.clip((dc * df).sum() / math.sqrt((dc * dc).sum()) / math.sqrt((df * df).sum()), -1.0, 1.0)) \
                if (dc * dc).sum() > 0 and (df * df).sum() > 0 else float("nan")
    return np.array([c.mean(), c.std(), c.max(), f.mean(), f.std(), f.max(), corr])


def tamper64(stats: np.ndarray) -> float:
    norm01 = lambda x, lo, hi: min(1.0, max(0.0, (x - lo) / (hi - lo + 1e-9)))
    return min(1.0, max(0.0, 0.6 * norm01(stats[0], 0.05, 0.5) + 0.4 * norm01(abs(stats[4] - stats[3]), 0.0, 0.5)))


def pooled64(g: np.ndarray) -> Dict[str, np.ndarray]:
    """Per pyramid chunk: mean and std of m in float64, max m (a float32 value), the 8 counts -> {"mean", "std", "max": (7,), "bins":
    (7, 8) int, "vector": (77,) float64 in the reference's order}.  Fewer than 2 frames: zeros."""
    pairs = len(g) - 1
    out = {"mean": np.zeros(7), "std": np.zeros(7), "max": np.zeros(7), "bins": np.zeros((7, 8), np.int64)}
    if pairs >= 1:
        d = diffs(g)
        for c, (lo, hi) in enumerate(chunks(pairs)):
            m, a = chunk_planes(d, lo, hi)
            m64 = m.astype(np.float64)
            out["mean"][c], out["std"][c], out["max"][c] = (m64.mean(), m64.std(), m64.max()) if hi > lo else (np.nan,) * 3
            out["bins"][c] = bins8(a)
    out["vector"] = np.concatenate([np.concatenate([[out["mean"][c], out["std"][c], out["max"][c]], out["bins"][c].astype(np.float64)]) for c in range(7)])
    return out


def tile_normalise64(v: np.ndarray, dim: int) -> np.ndarray:
    v = np.asarray(v, np.float64)
    t = np.tile(v, -(-dim // v.size))[:dim]
    return t / (np.linalg.norm(t) + 1e-9)


# ------------------------------------------------------------------ bounds (float32 evaluation against float64)
def sum_roundings(n: int) -> int:
    """Roundings on any path of NumPy's float32 sum of n values: below 8 values a plain loop (n - 1); otherwise blocks of up to 128
    values on 8 interleaved accumulators (block / 8 additions each, 3 levels to combine them, up to 7 leftover additions) and a
    pairwise tree over the blocks (ceil(log2(n / 128)) levels).  35 for a 65,536-pixel plane."""
    if n < 8:
        return max(n - 1, 0)
    return min(n, 128) // 8 + 3 + 7 + max(0, math.ceil(math.log2(n / 128)))


def mean_bound(mean: float, n: int) -> float:
    """|fl32 mean - mean| for n NON-NEGATIVE values: every rounding of the sum is relative to a partial sum <= the total, then one
    division: (sum_roundings + 1) u relative, first order; x 1.01 for the higher orders."""
    return 1.01 * (sum_roundings(n) + 1) * U32 * abs(mean)


def std_bound(std: float, mean: float, n: int) -> float:
    """|fl32 std - std|, NumPy's two-pass form.  The float32 mean is off by delta <= mean_bound; the exact second moment about a point
    delta off the mean is std^2 + delta^2.  Each term fl((x - mean')^2) carries 3 u (one subtraction, squared, one product), the sum
    sum_roundings u (non-negative terms), the division and the square root u each: var' = (std^2 + delta^2)(1 + theta), |theta| <=
    (sum_roundings + 4) u, and std' = sqrt(var')(1 + u).  With sqrt(std^2 + delta^2) <= std + delta:
        |std' - std| <= delta + (std + delta)((sum_roundings + 4) / 2 + 1) u          (x 1.01 for the higher orders)."""
    delta = mean_bound(mean, n)
    return 1.01 * (delta + (std + delta) * ((sum_roundings(n) + 4) / 2 + 1) * U32)


def corr_bound(cut: np.ndarray, flow: np.ndarray) -> float:
    """np.corrcoef works in float64 even on float32 series, so the reference's value is a float64 evaluation rounded to float32: u
    (|r| <= 1) plus the float64 evaluation's own error, which carries the series' conditioning kappa = max|x| / std: the deviations
    x - mean are known to 2^-53 kappa relative, the three sums of n products to n 2^-53 more: 8 n (kappa_c + kappa_f)^2 2^-53 covers it."""
    c, f = np.asarray(cut, np.float64), np.asarray(flow, np.float64)
    kc, kf = np.abs(c).max() / c.std(), np.abs(f).max() / f.std()
    return U32 + 8 * c.size * (kc + kf) ** 2 * 2.0 ** -53


def chronos_bounds(cut: np.ndarray, flow: np.ndarray) -> np.ndarray:
    """Bounds of the seven statistics for series whose float64 statistics are s: [mean, std, max (exact: one rounding of a float32
    value is none), ...]."""
    s, n = chronos_stats64(cut, flow), len(cut)
    cb = corr_bound(cut, flow) if n > 3 and np.isfinite(s[6]) else 0.0
    return np.array([mean_bound(s[0], n), std_bound(s[1], s[0], n), 0.0, mean_bound(s[3], n), std_bound(s[4], s[3], n), 0.0, cb])


def pooled_bounds(p: Dict[str, np.ndarray]) -> np.ndarray:
    """(77,) bounds of the pooled vector: mean and std of a plane of 65,536 non-negative values; max and counts are exact."""
    out = np.zeros(77)
    for c in range(7):
        if np.isfinite(p["mean"][c]):
            out[11 * c], out[11 * c + 1] = mean_bound(p["mean"][c], PLANE), std_bound(p["std"][c], p["mean"][c], PLANE)
    return out


def vector_bound(v64: np.ndarray, entry_bounds: np.ndarray, dim: int) -> float:
    """max |fl32(tile(v) / (norm + 1e-9)) - float64 of the same| when entry k of v is off by at most entry_bounds[k].  With N the
    norm of the tiled vector and E the norm of the tiled bounds: the numerator moves an entry by e_k / N, the norm moves by at most E
    (relative E / N), float32 norm = sqrt(dot): dim roundings on a sum of squares, worst case in any order, halved by the square
    root, plus the root, the 1e-9 addition and the division: (dim / 2 + 3) u relative.  So
        |delta out_j| <= e_j / N + |out_j| (E / N + (dim / 2 + 3) u)                  (x 1.01 for the higher orders)."""
    reps = -(-dim // v64.size)
    t, e = np.tile(np.asarray(v64, np.float64), reps)[:dim], np.tile(entry_bounds, reps)[:dim]
    N, E = np.linalg.norm(t), np.linalg.norm(e)
    if not np.isfinite(N) or N == 0:
        return 0.0
    return float(1.01 * np.max(e / N + np.abs(t) / N * (E / N + (dim / 2 + 3) * U32)))


def ulp_distance32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float32 ulps between two non-negative float32 arrays."""
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def load_fixture(path) -> Dict[str, Dict[str, np.ndarray]]:
    z = np.load(path)
    return {str(n): {k: z[f"{n}/{k}"] for k in ("frames", "cut_scores", "flows", "stats", "features", "tamper", "pooled", "flow256", "flow512")}
            for n in z["names"]}
