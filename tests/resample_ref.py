"""Mirror of audio.resample (csrc/resample.hip), NumPy only: the filter restated from its formulas, the NumPy fp32 channel mix,
the float64 direct sum with the fp32-rounded taps, the bound every summation order meets, and a float32 mirror of the declared chain
order (ascending tap index over each phase's stored band).

  y[q n + p] = sum_k h[p][k] xz[q o + k - width],   xz the mixed clip, zero outside [0, len),   m = ceil(n len / o) outputs
  bound:  |y - y64| <= (T_p + 1) 2^-24 sum_k |h[p][k]| |x_k|,  T_p the band length of phase p.  Each of the T_p products and T_p
          sums of a chain rounds once at most (a fused step: once), with relative error 2^-24 on a partial sum that
          sum |h| |x| bounds in magnitude -- the textbook bound for any order, fused or not, to first order.
"""
import math

import numpy as np

QUALITIES = {"kaiser_best": (64, 0.9475937167399596, 14.769656459379492), "kaiser_fast": (16, 0.85, 8.555504641634386), "hann": (6, 0.99, None)}
PAIRS_TO_16K = (44100, 48000, 22050, 8000, 32000, 11025, 24000)
PAIRS = tuple((r, 16000) for r in PAIRS_TO_16K) + ((16000, 44100),)
U = 2.0 ** -24


def taps_ref(orig_sr: int, new_sr: int, quality: str) -> dict:
    """The tap table from the formulas, written independently of the package: sin(pi t) / (pi t) for the sinc, the band by |t| < lpw."""
    g = math.gcd(orig_sr, new_sr)
    o, n = orig_sr // g, new_sr // g
    lpw, rolloff, beta = QUALITIES[quality]
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    K = 2 * width + o
    k = np.arange(K, dtype=np.int64)
    h64 = np.zeros((n, K))
    first, count = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for p in range(n):
        num = (k - width) * n - p * o
        t = num / (o * n) * base
        band = np.flatnonzero(np.abs(t) < lpw)
        first[p], count[p] = band[0], len(band)
        assert np.array_equal(band, np.arange(band[0], band[0] + len(band)))
        tb = t[band]
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(num[band] == 0, 1.0, np.sin(np.pi * tb) / (np.pi * tb))
        if beta is None:
            w = np.cos(np.pi * tb / (2 * lpw)) ** 2
        else:
            w = np.i0(beta * np.sqrt(1.0 - (tb / lpw) ** 2)) / np.i0(beta)
        h64[p, band] = (base / o) * sinc * w
    return {"o": o, "n": n, "width": width, "K": K, "h64": h64, "h": h64.astype(np.float32), "first": first, "count": count, "lpw": lpw}


def mix_ref(x: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """(T,) or (C, T) of any dtype -> mono float32: astype(float32), mean over the channels, one multiplication by scale."""
    x = np.asarray(x).astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=0)
    return (x * np.float32(scale)).astype(np.float32)


def resampled_length_ref(length: int, o: int, n: int) -> int:
    return -(-n * int(length) // o)


def _windows(x: np.ndarray, taps: dict, p: int, nq: int) -> np.ndarray:
    """(nq, count[p]) float64: row q = xz[q o + k - width] for the band's k."""
    o, width, f, c = taps["o"], taps["width"], int(taps["first"][p]), int(taps["count"][p])
    xz = np.zeros(width + nq * o + taps["K"] + 1)
    xz[width:width + len(x)] = x
    idx = np.arange(nq)[:, None] * o + f + np.arange(c)[None, :]      # (+ width - width)
    return xz[idx]


def resample_ref(x: np.ndarray, taps: dict):
    """mono float32 (T,) -> (y64, bound): the float64 direct sum with the fp32-rounded taps and the any-order fp32 bound."""
    o, n = taps["o"], taps["n"]
    m = resampled_length_ref(len(x), o, n)
    y, bound = np.zeros(m), np.zeros(m)
    x = np.asarray(x, dtype=np.float64)
    for p in range(min(n, m)):
        nq = -(-(m - p) // n)
        f, c = int(taps["first"][p]), int(taps["count"][p])
        hp = taps["h"][p, f:f + c].astype(np.float64)
        win = _windows(x, taps, p, nq)
        y[p::n] = win @ hp
        bound[p::n] = (c + 1) * U * (np.abs(win) @ np.abs(hp))
    return y, bound


def resample_chain_f32(x: np.ndarray, taps: dict) -> np.ndarray:
    """The declared chain in float32: acc = fl32(h x + acc) over the band in ascending k, from zero.  The product of two fp32 values
    is exact in float64; the sum rounds to float64 and then to float32, which can double-round where a true fmaf rounds once."""
    o, n = taps["o"], taps["n"]
    m = resampled_length_ref(len(x), o, n)
    y = np.zeros(m, dtype=np.float32)
    x = np.asarray(x, dtype=np.float64)
    for p in range(min(n, m)):
        nq = -(-(m - p) // n)
        f, c = int(taps["first"][p]), int(taps["count"][p])
        hp = taps["h"][p, f:f + c].astype(np.float64)
        win = _windows(x, taps, p, nq)
        acc = np.zeros(nq, dtype=np.float32)
        for k in range(c):
            acc = (hp[k] * win[:, k] + acc.astype(np.float64)).astype(np.float32)
        y[p::n] = acc
    return y


def upfirdn_prototype(taps: dict):
    """The interleaved prototype g and its delay: tap (p, k) at index p o - (k - width) n + shift, shift = (width + o - 1) n; then
    y[j] = upfirdn(g, x, up=n)[shift + j o]."""
    o, n, width, K = taps["o"], taps["n"], taps["width"], taps["K"]
    shift = (width + o - 1) * n
    g = np.zeros(shift + (n - 1) * o + width * n + 1)
    p, k = np.meshgrid(np.arange(n), np.arange(K), indexing="ij")
    g[p * o - (k - width) * n + shift] = taps["h"].astype(np.float64)
    return g, shift


def unpack_device_table(taps: dict) -> np.ndarray:
    """The package's device tables (groups of 4 phases of a super-stride of G strides) back to (n', K') dense taps."""
    G, groups, table, o, n, K = taps["G"], taps["groups"], taps["table"], taps["o"], taps["n"], taps["K"]
    k_pad = max(int((groups[:, 0] + groups[:, 1]).max()), K + (G - 1) * o)
    dense = np.zeros((4 * len(groups), k_pad), dtype=np.float32)
    for g, (lo, cnt, off) in enumerate(groups):
        dense[4 * g:4 * g + 4, lo:lo + cnt] = table[off:off + cnt].T
    return dense[:, :K + (G - 1) * o], dense[G * n:]


def tone_gain(taps: dict, orig_sr: int, freq: float, seconds: float = 0.05) -> float:
    """RMS amplitude (x sqrt 2) of a unit sine of `freq` Hz after the float64 mirror, over the middle half of the output."""
    t = np.arange(int(orig_sr * seconds)) / orig_sr
    y, _ = resample_ref(np.sin(2 * np.pi * freq * t), taps)
    mid = y[len(y) // 4:3 * len(y) // 4]
    return float(np.sqrt(2 * np.mean(mid ** 2)))
