"""Float64 mirror of the STFT audio forensics entries (csrc/spectral.hip), the error bounds derived from the kernel's arithmetic,
and a float32 mirror of the kernel's own summation order.  NumPy only.

The bound, stated once.  u = 2^-24 (the unit roundoff of fp32 round-to-nearest); A_t = sum |x_n| over the 400 taps of frame t.
  * The fp32 MFMA is a k-ordered fmaf chain (one rounding per product-and-add).  re and im of a bin are each ONE chain of 400 fmaf from
    zero, so each carries at most 400 roundings of partial sums that never exceed sum |x_n b_n| in magnitude (to first order):
    |d re| <= 400 u sum |x_n cos|,  |d im| <= 400 u sum |x_n sin|.
  * The basis is the float64 value rounded once: |d b_n| <= u |b_n|, one more u on each of the two sums.
  * | |S'| - |S| | <= |(d re, d im)| <= 401 u |(sum |x_n cos|, sum |x_n sin|)| <= 401 u A_t  (Minkowski: the vectors
    |x_n| (|cos|, |sin|) have length |x_n|).
  * |S| = sqrtf(fmaf(re, re, im im)): three roundings, each at most u relative to |S|^2 or |S|, together at most 3 u |S| <= 3 u A_t.
  C_CHAIN = 400 + 1 + 3 = 404:  | |S|_gpu - |S|_64 | <= 404 u A_t =: bin_bound[t], the same for every bin of frame t.
Folding the symmetric taps or splitting K would change the chain length and this constant with it; the kernel does neither.
Everything else follows from the per-bin bound d_t (all statistics are evaluated in double on the device and rounded to fp32 once):
  mean      mean_t d_t + u |mean|                     std   sqrt(mean_t d_t^2) + u std   (std is 1-Lipschitz in the RMS norm)
  max, min  max_t d_t   (compared at the mirror's VALUES: the positions may differ)
  mel_like  d_t + 3 u mel                              (two adds and a division in fp32 on non-negative terms)
  features  f = v / (|v| + 1e-9), v = the statistics tiled: 2 |dv| / (|v| + 1e-9) + 4 u |f_i|  (norm rounding, the 1e-9 add, the
            division, and one spare), |dv| from the four bounds above; an all-zero clip gives exactly zero
  energy    thread t of 256 chains ceil(n / 256) fmaf, then 8 adds of the tree and one division: (ceil(n / 256) + 10) u e;
  score     e / (e + 1) has slope <= 1: the energy bound + u score.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

N_FFT, HOP, BINS, PAD, BANDS, MIN_SAMPLES = 400, 160, 201, 200, 64, 201
U = 2.0 ** -24
C_CHAIN = 404
# the kernel's tap order: MFMA step (u, e) multiplies taps 8u + e (lanes 0-31) and 8u + 4 + e (lanes 32-63), in that order
TAP_ORDER = [8 * u + 4 * half + e for u in range(N_FFT // 8) for e in range(4) for half in range(2)]
GOLDEN = Path(__file__).resolve().parent / "golden" / "spectral.npz"


def frame_count(n: int) -> int:
    return 1 + n // HOP if n >= MIN_SAMPLES else 0


def mono(wave: np.ndarray) -> np.ndarray:
    """(T,) or (C, T) -> (T,) float32 as the reference's _ensure_mono_16k."""
    w = np.asarray(wave).astype(np.float32)
    return w.mean(axis=0) if w.ndim == 2 else w


def frames(x: np.ndarray) -> np.ndarray:
    """(T_b, 400): frame t = samples 160 t .. 160 t + 399 of the clip reflect-padded by 200 (torch.stft, center=True); dtype of x."""
    assert x.ndim == 1 and x.shape[0] >= MIN_SAMPLES
    xp = np.pad(x, PAD, mode="reflect")
    idx = HOP * np.arange(frame_count(x.shape[0]))[:, None] + np.arange(N_FFT)[None, :]
    return xp[idx]


def basis64() -> np.ndarray:
    """(402, 400) float64: cos(2 pi k n / 400) for k < 201, then -sin; the angle reduced exactly."""
    kn = (np.arange(BINS, dtype=np.int64)[:, None] * np.arange(N_FFT, dtype=np.int64)[None, :]) % N_FFT
    ang = 2.0 * np.pi * kn.astype(np.float64) / N_FFT
    return np.concatenate([np.cos(ang), -np.sin(ang)])


def magnitude64(x: np.ndarray) -> np.ndarray:
    """(201, T_b) float64: the direct DFT of the fp32 samples."""
    f = frames(x.astype(np.float32)).astype(np.float64)
    b = basis64()
    return np.hypot(f @ b[:BINS].T, f @ b[BINS:].T).T


def bin_bound(x: np.ndarray) -> np.ndarray:
    """(T_b,): C_CHAIN u sum |x_n| per frame."""
    return C_CHAIN * U * np.abs(frames(x.astype(np.float32)).astype(np.float64)).sum(axis=1)


def stats64(mag: np.ndarray) -> np.ndarray:
    return np.array([mag.mean(), mag.std(), mag.max(), mag.min()], dtype=np.float64)


def stats_bound(x: np.ndarray, st: np.ndarray) -> np.ndarray:
    d = bin_bound(x)
    return np.array([d.mean() + U * abs(st[0]), np.sqrt((d * d).mean()) + U * st[1], d.max(), d.max()])


def mel64(mag: np.ndarray) -> np.ndarray:
    return mag[:3 * BANDS].reshape(BANDS, 3, -1).mean(axis=1)


def mel_bound(x: np.ndarray, mel: np.ndarray) -> np.ndarray:
    return bin_bound(x)[None, :] + 3 * U * mel


def features64(st: np.ndarray, dim: int) -> np.ndarray:
    v = np.tile(st, -(-dim // 4))[:dim]
    return v / (np.linalg.norm(v) + 1e-9)


def features_bound(st: np.ndarray, st_bound: np.ndarray, dim: int) -> np.ndarray:
    v = np.tile(st, -(-dim // 4))[:dim]
    dv = np.linalg.norm(np.tile(st_bound, -(-dim // 4))[:dim])
    n = np.linalg.norm(v)
    if n == 0.0 and dv == 0.0:
        return np.zeros(dim)
    return 2.0 * dv / (n + 1e-9) + 4 * U * np.abs(features64(st, dim))


def energy64(x: np.ndarray) -> float:
    x = x.astype(np.float64)
    return float((x * x).mean()) if x.size else 0.0


def energy_bound(n: int, e: float) -> float:
    return (-(-n // 256) + 10) * U * e


def score64(e: float) -> float:
    return min(max(e / (e + 1.0), 0.0), 1.0)


def score_bound(n: int, e: float) -> float:
    return energy_bound(n, e) + U * score64(e)


def _fmaf(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp32 fused multiply-add through float64: the product of two fp32 is exact in float64; the sum is rounded to 53 bits and then to
    24 (a double rounding that differs from the fused result only on near-ties of the 53-bit sum)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def chain_magnitude32(x: np.ndarray, basis32: np.ndarray) -> np.ndarray:
    """(201, T_b) float32: the kernel's own arithmetic -- per (frame, bin) one fmaf chain over the taps in TAP_ORDER from zero for re
    and for im (basis32: the (402, 400) fp32 basis the kernel is given), then sqrtf(fmaf(re, re, im im))."""
    f = frames(x.astype(np.float32))
    re = np.zeros((f.shape[0], BINS), np.float32)
    im = np.zeros((f.shape[0], BINS), np.float32)
    for k in TAP_ORDER:
        a = f[:, k:k + 1]
        re = _fmaf(a, basis32[None, :BINS, k], re)
        im = _fmaf(a, basis32[None, BINS:, k], im)
    return np.sqrt(_fmaf(re, re, im * im)).T


def rel_l2(a: np.ndarray, ref: np.ndarray) -> float:
    d = np.linalg.norm(a.astype(np.float64) - ref)
    n = np.linalg.norm(ref)
    return float(d / n) if n > 0 else float(d)


def golden() -> dict:
    """The fixture as {clip name: {key: array}} (tests/golden/make_golden_spectral.py); waves come back as float32."""
    z = np.load(GOLDEN)
    out = {}
    for name in z["names"]:
        name = str(name)
        out[name] = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
        out[name]["wave"] = out[name]["wave"].astype(np.float32)
    return out
