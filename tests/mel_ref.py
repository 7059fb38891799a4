"""Float64 NumPy restatement of the reference's librosa-branch mel spectrogram in dB (src/core_blocks/audio_blocks.py:71-78:
power_to_db(melspectrogram(y, sr=16000, n_fft=400, hop_length=160, n_mels=64, power=2.0), ref=np.max)), the exact fp32 mirror of
the device's filterbank chain, and the bounds the device path (csrc/mel_db.hip) is held to.

librosa is not part of this environment: every definition here is RESTATED from librosa's documented algorithms (0.10 defaults) and
nothing is verified against librosa itself; no fixture of the reference exists for this branch for the same reason.  What IS checked
independently (tests/test_mel_ref.py): the filterbank against transformers.audio_utils.mel_filter_bank, the STFT against
scipy.signal.stft, the fmaf mirror against rational arithmetic.

Bounds.  u = 2^-24.  A magnitude of the device is within d_t = mag_bound (tests/librosa_ref.py) of float64.  S in
[max(S - d, 0), S + d] is carried through the monotone steps: the square; the non-negative weighted sum; the fp32 work on it, a
relative g = n u / (1 - n u) with n = count + 2 (the weight rounded once, the square rounded once, a chain of `count` fmaf over
non-negative terms), plus count 2^-149 W_max for products that underflow; the clip maximum; the logarithm (D rises with M and
falls with the maximum); the floor.  D is evaluated in double on the device and rounded once: a relative 2 u and 1e-12 on top.
Since M <= max M in any arithmetic that has a monotone log10, D <= 0 always: the upper end is cut there."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from librosa_ref import U, frame_counts, inside, mag_bound, stft_mag      # noqa: F401  (re-exported for the tests)

N_MELS, N_BINS, HOP, TILE = 64, 201, 160, 64
AMIN, TOP_DB = 1e-10, 80.0
MISTAKES = ("htk_scale", "no_slaney_norm", "magnitude_not_power", "ref_one", "per_frame_ref", "per_tile_ref", "no_floor", "floor_before_ref",
            "natural_log", "bin_shift", "edges_65")


# ----------------------------------------------------------------------------------------------------------------- the filterbank
def mel_of(f, htk: bool = False):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f >= 1000.0, 15.0 + 27.0 * np.log(np.maximum(f, 1000.0) / 1000.0) / np.log(6.4), 3.0 * f / 200.0)


def hz_of(m, htk: bool = False):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) * (np.maximum(m, 15.0) - 15.0) / 27.0), 200.0 * m / 3.0)


def mel_points(htk: bool = False, points: int = N_MELS + 2) -> np.ndarray:
    """66 points in Hz, equally spaced in mel over [mel(0), mel(8000)].  points=65 (the mistake `edges_65`): the spacing of 65 points
    over the range, continued to 66 points so that 64 triangles still come out."""
    top = float(mel_of(8000.0, htk))
    return hz_of(np.arange(N_MELS + 2) * (top / (points - 1)), htk) if points != N_MELS + 2 else hz_of(np.linspace(0.0, top, points), htk)


def filterbank(htk: bool = False, slaney_norm: bool = True, bin_shift: int = 0, points: int = N_MELS + 2) -> np.ndarray:
    """(64, 201) float64."""
    m = mel_points(htk, points)
    f = 40.0 * (np.arange(N_BINS) + bin_shift)
    W = np.zeros((N_MELS, N_BINS))
    for i in range(N_MELS):
        lower = (f - m[i]) / (m[i + 1] - m[i])
        upper = (m[i + 2] - f) / (m[i + 2] - m[i + 1])
        W[i] = np.maximum(0.0, np.minimum(lower, upper))
        if slaney_norm:
            W[i] *= 2.0 / (m[i + 2] - m[i])
    return W


def supports(W: np.ndarray):
    """(first, count) per row; asserts the supports are contiguous."""
    first = np.array([np.flatnonzero(r)[0] for r in W])
    count = np.array([np.count_nonzero(r) for r in W])
    for i, r in enumerate(W):
        assert r[first[i]:first[i] + count[i]].all(), i
    return first, count


# ----------------------------------------------------------------------------------------------------------------- the restatement
def power_to_db(M: np.ndarray, ref, log=np.log10, floor: bool = True) -> np.ndarray:
    """librosa.power_to_db(M, ref=ref, amin=1e-10, top_db=80): ref is a value or an array that broadcasts against M."""
    L = 10.0 * log(np.maximum(AMIN, M)) - 10.0 * log(np.maximum(AMIN, ref))
    return np.maximum(L, L.max() - TOP_DB) if floor and L.size else L


def mel_db(x: np.ndarray, mistake: str = None) -> dict:
    """{"mel_power": (64, T), "mel_db": (64, T), "mel_max"} of one clip of at least one sample, in float64.  `mistake`: one of
    MISTAKES, applied to the restatement (the table that shows the bounds are not vacuous)."""
    assert mistake is None or mistake in MISTAKES, mistake
    x = np.asarray(x, dtype=np.float32)
    S = stft_mag(x, "A")
    W = filterbank(htk=mistake == "htk_scale", slaney_norm=mistake != "no_slaney_norm", bin_shift=int(mistake == "bin_shift"),
                   points=65 if mistake == "edges_65" else N_MELS + 2)
    M = W @ (S if mistake == "magnitude_not_power" else S * S)
    log = np.log if mistake == "natural_log" else np.log10
    if mistake == "ref_one":
        D = power_to_db(M, 1.0, log)
    elif mistake == "per_frame_ref":
        D = power_to_db(M, M.max(axis=0, keepdims=True), log)
    elif mistake == "per_tile_ref":
        ref = np.concatenate([np.full(M[:, t:t + TILE].shape, M[:, t:t + TILE].max()) for t in range(0, M.shape[1], TILE)], axis=1)
        D = power_to_db(M, ref, log)
    elif mistake == "no_floor":
        D = power_to_db(M, M.max(), log, floor=False)
    elif mistake == "floor_before_ref":      # the floor taken on 10 log10 M itself, the reference subtracted afterwards
        D = np.maximum(10.0 * log(np.maximum(AMIN, M)), -TOP_DB) - 10.0 * log(np.maximum(AMIN, M.max()))
    else:
        D = power_to_db(M, M.max(), log)
    return {"mel_power": M, "mel_db": D, "mel_max": M.max()}


# ----------------------------------------------------------------------------------------------------------------- the exact mirror
def fma32(a, b, c) -> np.ndarray:
    """fmaf(a, b, c) of float32 arrays, exactly: one rounding of the exact a b + c.  The product of two float32 is exact in float64.
    The float64 sum s = fl(p + c) is NOT the exact value, and rounding it to float32 rounds twice: wrong exactly when s sits on a
    float32 tie (the midpoint of two neighbours, which float64 represents) while the exact sum does not.  The two-sum residual
    e = (p + c) - s, itself exact, says on which side of the tie the exact sum lies.  (If s is no tie, no float32 midpoint lies
    between s and the exact sum -- it would be a float64 nearer to the exact sum than s -- so rounding s is right.)"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
        d = s - r64
        fix_up = (d > 0) & (2.0 * d == up.astype(np.float64) - r64) & (e > 0)
        fix_dn = (d < 0) & (-2.0 * d == r64 - dn.astype(np.float64)) & (e < 0)
    return np.where(fix_up, up, np.where(fix_dn, dn, r)).astype(np.float32)


def fma32_naive(a, b, c) -> np.ndarray:
    """The mirror that rounds twice (float64 sum, then float32): what fma32 replaces."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def round32(q: Fraction) -> np.float32:
    """The float32 nearest to the rational q, ties to even, by exact comparison."""
    r = np.float32(float(q))
    cands = [r, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))]
    dist = [abs(Fraction(float(v)) - q) for v in cands]
    best = min(dist)
    tied = [v for v, dv in zip(cands, dist) if dv == best]
    if len(tied) > 1:
        tied = [v for v in tied if (v.view(np.uint32) & 1) == 0]
    return tied[0]


def mel_power_mirror(S32: np.ndarray, weights32: np.ndarray, first, count) -> np.ndarray:
    """The device chain on ITS magnitudes: P = S S in float32, M[i] = one chain of fmaf from zero over row i's support in ascending
    bins.  (64, T) float32, every bit."""
    S32 = np.asarray(S32, dtype=np.float32)
    P = S32 * S32
    M = np.zeros((N_MELS, S32.shape[1]), dtype=np.float32)
    for i in range(N_MELS):
        for k in range(int(first[i]), int(first[i]) + int(count[i])):
            M[i] = fma32(weights32[i, k], P[k], M[i])
    return M


def db_of_device(M32: np.ndarray, mx32) -> np.ndarray:
    """The dB formula in float64 on the device's own powers and maximum."""
    return np.maximum(10.0 * np.log10(np.maximum(AMIN, M32.astype(np.float64))) - 10.0 * np.log10(max(AMIN, float(mx32))), -TOP_DB)


# ----------------------------------------------------------------------------------------------------------------- the bounds
def bounds(x: np.ndarray) -> dict:
    """{"center": mel_db(x), "mel_power": (lo, hi), "mel_max": (lo, hi), "mel_db": (lo, hi)} (module docstring)."""
    x = np.asarray(x, dtype=np.float32)
    c = mel_db(x)
    S = stft_mag(x, "A")
    d = mag_bound(x, "A")[None, :]
    Slo, Shi = np.maximum(S - d, 0.0), S + d
    W = filterbank()
    _, count = supports(W)
    n = (count + 2.0)[:, None]
    g = n * U / (1.0 - n * U)
    tiny = (count * 2.0 ** -149 * W.max())[:, None]
    Mlo = np.maximum((W @ (Slo * Slo)) * (1.0 - g) - tiny, 0.0)
    Mhi = (W @ (Shi * Shi)) * (1.0 + g) + tiny
    xlo, xhi = Mlo.max(), Mhi.max()

    def db(M, mx):
        return np.maximum(10.0 * np.log10(np.maximum(AMIN, M)) - 10.0 * np.log10(max(AMIN, mx)), -TOP_DB)

    Dlo, Dhi = db(Mlo, xhi), np.minimum(db(Mhi, xlo), 0.0)
    Dlo, Dhi = Dlo - 2 * U * np.abs(Dlo) - 1e-12, Dhi + 2 * U * np.abs(Dhi) + 1e-12
    return {"center": c, "mel_power": (Mlo, Mhi), "mel_max": (xlo, xhi), "mel_db": (Dlo, Dhi)}


def outside_names(values: dict, b: dict):
    return [k for k in ("mel_power", "mel_max", "mel_db") if k in values and not inside(values[k], b[k]).all()]


# ----------------------------------------------------------------------------------------------------------------- the cases
def cases() -> dict:
    """1 s of white noise at 0.1; the same with its second half zeroed (the floor is live); a 440 Hz tone (most entries floored);
    quiet_then_loud: 130 frames, noise at 1e-3 up to the last 64-frame tile's first sample, 0.5 from there on (a per-tile reference
    is off by 54 dB on the first tile); an all-zero clip."""
    rng = np.random.default_rng(64)
    noise = (0.1 * rng.standard_normal(16000)).astype(np.float32)
    half = noise.copy()
    half[8000:] = 0.0
    tone = (0.5 * np.sin(2.0 * np.pi * 440.0 * np.arange(16000) / 16000.0)).astype(np.float32)
    ql = (1e-3 * rng.standard_normal(129 * HOP)).astype(np.float32)
    ql[128 * HOP:] = (0.5 * rng.standard_normal(HOP)).astype(np.float32)
    return {"noise": noise, "half_silent": half, "tone440": tone, "quiet_then_loud": ql, "zeros": np.zeros(4000, dtype=np.float32)}
