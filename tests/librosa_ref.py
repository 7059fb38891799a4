"""Float64 NumPy restatement of the reference's librosa branches (src/core_blocks/audio_blocks.py:141-176, :244-254) and the bounds
the device path (csrc/spectral_desc.hip) is held to.

librosa is not part of this environment: every definition here is RESTATED from librosa's documented algorithms (0.10 defaults) and
nothing is verified against librosa itself; no fixture of the reference exists for this branch for the same reason.  What IS checked
independently: both STFT geometries against scipy.signal.stft (tests/test_librosa_ref.py).

Bounds.  u = 2^-24.  A magnitude of the device is within  d_t = (n_fft + 1) u sum_n |w[n] x_pad[hop t + n]|  of float64: the basis
w cos / w sin is rounded once (u) and re, im are chains of n_fft fmaf (n_fft u, first order), and the error vector (e_re, e_im) is no
longer than (n_fft + 1) u sum_n |w x| (|cos|, |sin|)_n, whose length is at most (n_fft + 1) u sum_n |w x| (triangle inequality).
Every later value is bounded by INTERVAL evaluation: S in [max(S - d, 0), S + d] is carried through the monotone pieces (order
statistics, log, means, the clip), and through Lipschitz bounds where a piece is not monotone (std, centroid).  Discrete choices
(the rolloff bin, which rows are the smallest, the `tiny` switch of the centroid) become possible SETS: an interval of bins, the
interval of an order statistic, the union of both branches.  On top of each interval comes the slack for the float32 arithmetic of
the reference's NumPy reductions, bounded for ANY summation order: a float32 sum of n terms is within n u sum|terms| of exact."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
SR = 16000
GEOMETRY = {"A": (400, 160), "B": (2048, 512)}
OCTA = (0.0, 200.0, 400.0, 800.0, 1600.0, 3200.0, 6400.0, 12800.0)
TINY32 = float(np.finfo(np.float32).tiny)
ZC_THRESHOLD = np.float32(1e-10)
DESCRIPTORS = ("mean", "std", "max", "min", "contrast_mean", "contrast_std", "flatness_mean", "flatness_std", "centroid", "rolloff", "zcr")
MISTAKES = ("rect_window", "reflect_pad", "band_edge", "idx_plus_one", "keep_last_row", "no_clip", "flatness_of_magnitude", "rolloff_le",
            "zcr_zero_pad")


# ----------------------------------------------------------------------------------------------------------------- the restatement
def frame_counts(n: int):
    return (1 + n // 160, 1 + n // 512) if n >= 1 else (0, 0)


def window(n_fft: int, kind: str = "hann") -> np.ndarray:
    """scipy.signal.get_window('hann', n_fft, fftbins=True): the periodic Hann window."""
    if kind == "rect":
        return np.ones(n_fft)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def framed(x: np.ndarray, n_fft: int, hop: int, pad: str = "zero") -> np.ndarray:
    """(T, n_fft) float64 frames of the clip padded by n_fft / 2 on both sides; T = 1 + len // hop."""
    x = np.asarray(x, dtype=np.float64)
    mode = {"zero": "constant", "reflect": "reflect", "edge": "edge"}[pad]
    if mode == "reflect" and len(x) <= n_fft // 2:
        mode = "constant"      # (numpy refuses a reflection longer than the clip; the mistake table never needs it)
    xp = np.pad(x, n_fft // 2, mode=mode)
    T = 1 + len(x) // hop
    return np.lib.stride_tricks.as_strided(xp, (T, n_fft), (hop * xp.strides[0], xp.strides[0])).copy()


def stft_mag(x: np.ndarray, which: str, window_kind: str = "hann", pad: str = "zero") -> np.ndarray:
    """|librosa.stft(x, n_fft, hop_length)|: (bins, T) float64."""
    n_fft, hop = GEOMETRY[which]
    return np.abs(np.fft.rfft(framed(x, n_fft, hop, pad) * window(n_fft, window_kind)[None, :], axis=1)).T


def mag_bound(x: np.ndarray, which: str) -> np.ndarray:
    """(T,): (n_fft + 1) u sum |w x| per frame."""
    n_fft, hop = GEOMETRY[which]
    return (n_fft + 1) * U * (np.abs(framed(x, n_fft, hop)) * window(n_fft)[None, :]).sum(axis=1)


def band_table(edge_shift: int = 0, idx_add: int = 0, drop_last: bool = True):
    """spectral_contrast's bands for sr 16000, n_fft 400: per band (rows used, idx).  The keywords are the named mistakes."""
    freq = np.arange(201) * 40.0
    out = []
    for k, (lo, hi) in enumerate(zip(OCTA[:-1], OCTA[1:])):
        band = (freq >= lo) & (freq <= hi)
        if edge_shift:
            band = np.roll(band, edge_shift)
            band[:edge_shift] = False
        idx = np.flatnonzero(band)
        if k > 0:
            band[idx[0] - 1] = True
        if k == 6:
            band[idx[-1] + 1:] = True
        rows = np.flatnonzero(band)
        if k < 6 and drop_last:
            rows = rows[:-1]
        out.append((rows, int(max(np.rint(0.02 * band.sum()), 1)) + idx_add))
    return out


def peaks_valleys(S: np.ndarray, table=None):
    """(7, T) each: mean of the idx largest / idx smallest rows of every band."""
    table = band_table() if table is None else table
    T = S.shape[1]
    peak, valley = np.zeros((7, T)), np.zeros((7, T))
    for k, (rows, idx) in enumerate(table):
        srt = np.sort(S[rows], axis=0)
        valley[k] = srt[:idx].mean(axis=0)
        peak[k] = srt[-idx:].mean(axis=0)
    return peak, valley


def power_to_db(v: np.ndarray, clip: bool = True, ref_max=None) -> np.ndarray:
    """10 log10(max(1e-10, v)), clipped from below at the array's own maximum - 80 (ref_max: that maximum, for interval ends)."""
    db = 10.0 * np.log10(np.maximum(1e-10, v))
    if clip and db.size:
        db = np.maximum(db, (db.max() if ref_max is None else ref_max) - 80.0)
    return db


def contrast(S: np.ndarray, table=None, clip: bool = True) -> np.ndarray:
    peak, valley = peaks_valleys(S, table)
    return power_to_db(peak, clip) - power_to_db(valley, clip)


def flatness(S: np.ndarray, power: bool = True) -> np.ndarray:
    """(T,): exp(mean log P) / mean P over the bins, P = max(1e-10, S^2)."""
    P = np.maximum(1e-10, S ** 2 if power else S)
    return np.exp(np.log(P).mean(axis=0)) / P.mean(axis=0)


def centroid(S: np.ndarray) -> np.ndarray:
    f = np.arange(S.shape[0]) * (SR / 2048.0)
    tot = S.sum(axis=0)
    return np.where(tot < TINY32, 0.0, (f[:, None] * S).sum(axis=0) / np.where(tot < TINY32, 1.0, tot))


def rolloff_bin(S: np.ndarray, le: bool = False) -> np.ndarray:
    """(T,) float: the first bin whose running sum is not below (mistake `le`: above) 0.85 of the total; NaN if there is none."""
    cum = np.cumsum(S, axis=0)
    thr = 0.85 * cum[-1]
    ok = cum > thr[None, :] if le else cum >= thr[None, :]
    return np.where(ok.any(axis=0), ok.argmax(axis=0), np.nan)


def zcr_counts(x: np.ndarray, pad: str = "edge") -> np.ndarray:
    """(T_B,) int: sign changes inside every 2048-sample frame of the padded clip; |x| <= float32(1e-10) counts as +0."""
    x = np.asarray(x, dtype=np.float32)
    neg = np.where(np.abs(x) <= ZC_THRESHOLD, False, np.signbit(x))
    fr = framed(neg.astype(np.float64), 2048, 512, pad) > 0.5
    return (fr[:, 1:] != fr[:, :-1]).sum(axis=1)


def features_of(desc: np.ndarray, dim: int) -> np.ndarray:
    v = np.tile(desc, -(-dim // len(desc)))[:dim]
    return v / (np.linalg.norm(v) + 1e-9)


def clone_of(flat_y: float, zcr: float, cent: float) -> float:
    return float(np.clip(0.4 * flat_y + 0.3 * zcr + 0.3 * np.tanh(cent / 3000.0), 0.0, 1.0))


def describe(x: np.ndarray, mistake: str = None) -> dict:
    """Every value of the device path for one clip of at least one sample, in float64.  `mistake`: one of MISTAKES, applied to
    the restatement (the table that shows the bounds are not vacuous)."""
    assert mistake is None or mistake in MISTAKES, mistake
    x = np.asarray(x, dtype=np.float32)
    wk = "rect" if mistake == "rect_window" else "hann"
    pad = "reflect" if mistake == "reflect_pad" else "zero"
    SA, SB = stft_mag(x, "A", wk, pad), stft_mag(x, "B", wk, pad)
    table = band_table(edge_shift=int(mistake == "band_edge"), idx_add=int(mistake == "idx_plus_one"), drop_last=mistake != "keep_last_row")
    o = {"magnitude": SA, "magnitude_y": SB}
    o["contrast"] = contrast(SA, table, clip=mistake != "no_clip")
    o["flatness"] = flatness(SA, power=mistake != "flatness_of_magnitude")
    o["centroid"] = centroid(SB)
    o["rolloff"] = rolloff_bin(SB, le=mistake == "rolloff_le") * (SR / 2048.0)
    o["flatness_y"] = flatness(SB, power=mistake != "flatness_of_magnitude")
    o["zc"] = zcr_counts(x, pad="zero" if mistake == "zcr_zero_pad" else "edge")
    o["zcr"] = o["zc"] / 2048.0
    o["descriptors"] = np.array([SA.mean(), SA.std(), SA.max(), SA.min(), o["contrast"].mean(), o["contrast"].std(), o["flatness"].mean(),
                                 o["flatness"].std(), o["centroid"].mean(), o["rolloff"].mean(), o["zcr"].mean()])
    o["clone_score"] = clone_of(o["flatness_y"].mean(), o["zcr"].mean(), o["centroid"].mean())
    return o


# ----------------------------------------------------------------------------------------------------------------- the bounds
def _wide(lo, hi, rel, abs_=0.0):
    """The interval after float32 work of relative size `rel` (at least the device's own final rounding, 2 u) and absolute `abs_`."""
    rel = np.maximum(rel, 2 * U)
    return lo - rel * np.abs(lo) - abs_, hi + rel * np.abs(hi) + abs_


def _mean_iv(lo, hi, axis=None):
    """Mean of n interval entries, float32 in any order: n u relative to the mean of |entries|."""
    n = lo.size if axis is None else lo.shape[axis]
    slack = n * U * np.maximum(np.abs(lo), np.abs(hi)).mean(axis=axis)
    return lo.mean(axis=axis) - slack - 2 * U * np.abs(lo.mean(axis=axis)), hi.mean(axis=axis) + slack + 2 * U * np.abs(hi.mean(axis=axis))


def _std_iv(center, lo, hi):
    """std is 1-Lipschitz in the RMS norm: |std(c + e) - std(c)| <= rms(e); float32 two-pass slack on top."""
    n = center.size
    rad = np.sqrt(np.mean(np.maximum(hi - center, center - lo) ** 2))
    s = center.std()
    amax = np.maximum(np.abs(lo), np.abs(hi)).max() if n else 0.0
    slack = (n + 4) * U * s + 2 * U * amax + n * U * np.abs(center).mean()
    return max(s - rad - slack, 0.0), s + rad + slack


def _flat_iv(Slo, Shi):
    """exp(mean log P) / mean P is increasing in the geometric and decreasing in the arithmetic mean, each monotone in S.  Slack for
    float32: log P and its mean within (n + 3) u max|log P| + 4 u, the arithmetic mean and the division within (n + 4) u."""
    n = Slo.shape[0]
    Plo, Phi = np.maximum(1e-10, Slo ** 2), np.maximum(1e-10, Shi ** 2)
    llo, lhi = np.log(Plo), np.log(Phi)
    e = (n + 3) * U * np.maximum(np.abs(llo), np.abs(lhi)).max(axis=0) + 4 * U
    r = (n + 4) * U
    lo = np.exp(llo.mean(axis=0) - e) / Phi.mean(axis=0) * (1 - r)
    hi = np.minimum(np.exp(lhi.mean(axis=0) + e) / Plo.mean(axis=0), 1.0) * (1 + r)
    return lo, hi


def _db_iv(vlo, vhi):
    """power_to_db with its clip on interval ends: monotone in the value and in the array's maximum; float32 log10 slack."""
    dlo, dhi = 10.0 * np.log10(np.maximum(1e-10, vlo)), 10.0 * np.log10(np.maximum(1e-10, vhi))
    dlo, dhi = np.maximum(dlo, dlo.max() - 80.0), np.maximum(dhi, dhi.max() - 80.0)
    slack = 4 * U * (np.maximum(np.abs(dlo), np.abs(dhi)) + 10.0)
    return dlo - slack, dhi + slack


def bounds(x: np.ndarray, dim: int = 128) -> dict:
    """name -> (lo, hi) for every value of describe(x) that carries rounding ("zc" is exact and has none; "rolloff_bins" is the
    possible set of the discrete choice, an inclusive interval of bins per frame), plus "center": describe(x) itself."""
    x = np.asarray(x, dtype=np.float32)
    c = describe(x)
    b = {"center": c}
    iv = {}
    for which, name in (("A", "magnitude"), ("B", "magnitude_y")):
        d = mag_bound(x, which)[None, :]
        iv[which] = (np.maximum(c[name] - d, 0.0), c[name] + d)
        b[name] = (c[name] - d, c[name] + d)
    # ---- path A
    Slo, Shi = iv["A"]
    SA = c["magnitude"]
    mean = _mean_iv(Slo, Shi)
    b["stats"] = [mean, _std_iv(SA, Slo, Shi), (Slo.max(), Shi.max()), (Slo.min(), Shi.min())]
    (plo, vlo), (phi, vhi) = peaks_valleys(Slo), peaks_valleys(Shi)      # order statistics are monotone in every entry
    plo, phi = _wide(plo, phi, 2 * U)
    vlo, vhi = _wide(vlo, vhi, 2 * U)
    (pdl, pdh), (vdl, vdh) = _db_iv(plo, phi), _db_iv(vlo, vhi)
    clo, chi = pdl - vdh, pdh - vdl
    clo, chi = _wide(clo, chi, 2 * U, 4 * U)
    b["contrast"] = (clo, chi)
    b["contrast_mean"], b["contrast_std"] = _mean_iv(clo, chi), _std_iv(c["contrast"], clo, chi)
    flo, fhi = _flat_iv(Slo, Shi)
    b["flatness"] = (flo, fhi)
    b["flatness_mean"], b["flatness_std"] = _mean_iv(flo, fhi), _std_iv(c["flatness"], flo, fhi)
    # ---- path B
    Slo, Shi = iv["B"]
    SB = c["magnitude_y"]
    n, hz = SB.shape[0], SR / 2048.0
    f = np.arange(n) * hz
    # centroid: c' - c = sum_k (f_k - c)(S'_k - S_k) / sum S'; both branches of the `tiny` switch where the total may be below it
    d = (Shi - SB)[0]
    tot_lo = Slo.sum(axis=0)
    cen = c["centroid"]
    safe = tot_lo > 2 * TINY32
    rad = np.where(safe, d * np.abs(f[:, None] - cen[None, :]).sum(axis=0) / np.where(safe, tot_lo, 1.0), 0.0)
    cl, ch = np.where(safe, cen - rad, 0.0), np.where(safe, cen + rad, f[-1])
    cl, ch = _wide(np.maximum(cl, 0.0), np.minimum(ch, f[-1]), 2 * n * U)
    b["centroid"] = (cl, ch)
    # rolloff: g_k = 0.15 sum_{j <= k} S_j - 0.85 sum_{j > k} S_j is increasing in the first sums and decreasing in the rest; bin k
    # certainly qualifies when its lowest value is above the float32 running sum's slack m, and cannot when its highest is below -m
    clo_, chi_ = np.cumsum(Slo, axis=0), np.cumsum(Shi, axis=0)
    g_lo = 0.15 * clo_ - 0.85 * (chi_[-1][None, :] - chi_)
    g_hi = 0.15 * chi_ - 0.85 * (clo_[-1][None, :] - clo_)
    m = 2 * n * U * chi_[-1][None, :]
    may, must = g_hi >= -m, g_lo > m
    kmin = may.argmax(axis=0)
    kmax = np.where(must.any(axis=0), must.argmax(axis=0), n - 1)
    b["rolloff_bins"] = (kmin, kmax)
    b["rolloff"] = (kmin * hz, kmax * hz)
    ylo, yhi = _flat_iv(Slo, Shi)
    b["flatness_y"] = (ylo, yhi)
    z = c["zcr"]
    b["zcr"] = (z, z)      # exact
    means = {k: _mean_iv(*b[k]) for k in ("centroid", "rolloff", "flatness_y", "zcr")}
    # ---- the 11 descriptors, the features and the clone score
    dlo = np.array([v[0] for v in b["stats"]] + [b["contrast_mean"][0], b["contrast_std"][0], b["flatness_mean"][0], b["flatness_std"][0],
                                                 means["centroid"][0], means["rolloff"][0], means["zcr"][0]])
    dhi = np.array([v[1] for v in b["stats"]] + [b["contrast_mean"][1], b["contrast_std"][1], b["flatness_mean"][1], b["flatness_std"][1],
                                                 means["centroid"][1], means["rolloff"][1], means["zcr"][1]])
    b["descriptors"] = (dlo, dhi)
    # features: f = v / N with N = |v| + 1e-9; |f - f0| <= r / (N0 - R) + |v0| R / (N0 (N0 - R)), R the norm of the tiled radii
    d0 = c["descriptors"]
    reps = -(-dim // 11)
    v0, r = np.tile(d0, reps)[:dim], np.tile(np.maximum(dhi - d0, d0 - dlo), reps)[:dim]
    N0, R = np.linalg.norm(v0) + 1e-9, np.linalg.norm(r)
    fb = r / (N0 - R) + np.abs(v0) * R / (N0 * (N0 - R)) + 8 * U if N0 > R else np.full(dim, 2.0)
    f0 = features_of(d0, dim)
    b["features"] = (f0 - fb, f0 + fb)
    # clone score: increasing in all three means
    lo = clone_of(means["flatness_y"][0], means["zcr"][0], means["centroid"][0])
    hi = clone_of(means["flatness_y"][1], means["zcr"][1], means["centroid"][1])
    b["clone_score"] = (lo - 8 * U, hi + 8 * U)
    return b


def inside(v, iv) -> np.ndarray:
    """Elementwise lo <= v <= hi; a NaN is outside."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= iv[0]) & (v <= iv[1])


CHECKED = ("magnitude", "magnitude_y", "contrast", "flatness", "centroid", "rolloff", "flatness_y", "zcr", "descriptors", "clone_score")


def outside_names(values: dict, b: dict):
    """Names of CHECKED whose values leave their bounds somewhere ("zc": the exact counts differ)."""
    out = [k for k in CHECKED if not inside(values[k], b[k]).all()]
    if not np.array_equal(values["zc"], b["center"]["zc"]):
        out.append("zc")
    return out


# ----------------------------------------------------------------------------------------------------------------- the cases
def cases() -> dict:
    """Seeded clips: white noise, a tone over a noise floor, silence, and exact zeros with +-1e-10 beside noise."""
    rng = np.random.default_rng(2024)
    t = np.arange(6000)
    gate = np.zeros(5000, dtype=np.float32)      # silence (whole frames of both STFTs), then noise: the 80 dB clip is live
    gate[3000:] = 0.2 * rng.standard_normal(2000)
    edge = 0.1 * rng.standard_normal(3000).astype(np.float32)
    edge[::7] = 0.0
    edge[1::7] = 1e-10
    edge[2::7] = -1e-10
    edge[3::7] = np.nextafter(np.float32(1e-10), np.float32(1))
    edge[4::7] = -np.nextafter(np.float32(1e-10), np.float32(1))
    edge[5::7] = -0.0
    neg = (0.1 * rng.standard_normal(2049)).astype(np.float32)
    neg[0] = -abs(neg[0]) - 0.01      # a negative first sample: edge padding and zero padding count differently
    return {"noise2049": neg, "noise4000": (0.1 * rng.standard_normal(4000)).astype(np.float32),
            "tone6000": (0.3 * np.sin(2 * np.pi * 1000.0 * t / SR) + 0.05 * rng.standard_normal(6000)).astype(np.float32),
            "silent3000": np.zeros(3000, dtype=np.float32), "gate5000": gate, "edge3000": edge}
