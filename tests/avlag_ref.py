"""Float64 NumPy restatement of the reference's estimate_av_lag (TemporalSyncNet, src/core_blocks/temporal_blocks.py:176-223, and
ChronosGuard, src/models/chronos_guard.py:175-196) as a DIRECT window, the exact fp32 mirror of the device's summation order
(csrc/av_lag.hip, include/ultrafnd_hip.h) and the radii the device path is held to.  The reference itself is the oracle here:
tests/golden/avlag.npz holds what its two functions returned (tests/golden/make_golden_avlag.py).

The window.  n = min(len a, len m); n < 4: 0.0.  ahat = (a - mean) / (std + 1e-9) (population std), mhat likewise;
K = int(max_lag_s * sr), Kc = min(K, n - 1);  c[k] = sum_i ahat[i + k] mhat[i] over the i with both indices in 0 .. n - 1,
k = -Kc .. Kc;  lag = the first argmax;  seconds = lag / sr.  (np.correlate(ahat, mhat, "full")[n - 1 + k] is c[k].)

The device's order (the mirror is written from the header's text).  Statistics in double: thread t of 1024 adds x[t], x[t + 1024], ...
in ascending order, the 1024 partials fold by halves (o = 512 .. 1: red[t] += red[t + o]); mean = sum / n, then the same for
(x - mean)^2, std = sqrt(sumsq / n); both rounded to fp32; xhat = (x - mean32) / (std32 + 1e-9f) in fp32.  Correlation: segments of
2048 samples i; P[s][k] = one fmaf chain from +0 over the segment's i in ascending order (terms outside the pair are zeros);
c[k] = ((P[0] + P[1]) + ...) + P[S - 1] + 0.0f in fp32.

Radii, u = 2^-24 (derived, not tuned).  With N_i = x_i - mu, D = sigma + 1e-9 (float64 from the raw input):
  mean    |mean32 - mu| <= e_mu = u |mu| + 2 d,  d = n 2^-52 max|x| (the double accumulation; the rounding to fp32)
  numer   |fl(x_i - mean32) - N_i| <= e_N = e_mu + u (|N_i| + e_mu)
  denom   |fl(std32 + 1e-9f) - D| <= e_D = u sigma + 2 n 2^-52 sigma (std32) + u 1e-9 (the fp32 constant) + u (D + that) (the sum)
  xhat    |xhat_i - N_i / D| <= e_i = q_i + u (|N_i| / D + q_i),  q_i = e_N / (D - e_D) + |N_i| e_D / (D (D - e_D))
  c[k]    |c_dev[k] - c[k]| <= g sum_i (|ahat| + e_a)[i + k] (|mhat| + e_m)[i]          the chain: g = L u / (1 - L u),
                                                                                         L = min(n, 2048) + (S - 1) + 1
                             + sum_i (e_a[i + k] |mhat_i| + |ahat[i + k]| e_m[i] + e_a[i + k] e_m[i])      the propagated error
          (the four sums are correlations of non-negative series, evaluated by a float64 FFT: 1e-9 (1 + value) is added for it, and
           1e-9 (1 + |c[k]|) for the restatement itself, which sums directly up to 5000 samples and by a float64 FFT above)
  peak    c[k] / n: radius[k] / n + u (|c[k]| + radius[k]) / n."""
from __future__ import annotations

import numpy as np

from mel_ref import fma32

U = 2.0 ** -24
SEG, LAG_BLOCK, WAVE_LAGS, ROW_THREADS = 2048, 1024, 512, 1024
DIRECT_MAX = 5000      # window64 sums directly up to this n
MISTAKES = ("sign_flipped", "swapped", "centre_off_by_one", "window_not_clamped", "ties_highest", "no_mean_removal", "longer_input", "k_from_fps",
            "ddof1")


def _f32(x) -> np.ndarray:
    return np.asarray(x).astype(np.float32).ravel()


def max_lag(sr: float, max_lag_s: float) -> int:
    return int(max_lag_s * sr)


# ----------------------------------------------------------------------------------------------------------------- the restatement
def standardise64(x: np.ndarray, ddof: int = 0, remove_mean: bool = True) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean() if remove_mean else 0.0
    sd = np.sqrt(((x - x.mean()) ** 2).sum() / max(x.size - ddof, 1))
    return (x - mu) / (sd + 1e-9)


def window64(a, m, K: int, mistake: str = None) -> dict:
    """{"n", "Kc", "c": c[-Kc .. Kc], "a_std", "m_std"} in float64 from the raw inputs; None for n < 4."""
    a, m = _f32(a), _f32(m)
    if mistake == "swapped":
        a, m = m, a
    n = min(a.size, m.size)
    if mistake == "longer_input":      # both brought to the LONGER length, the shorter one zero-padded
        n = max(a.size, m.size)
        a, m = np.pad(a, (0, n - a.size)), np.pad(m, (0, n - m.size))
    if n < 4:
        return None
    ddof, rm = int(mistake == "ddof1"), mistake != "no_mean_removal"
    ah, mh = standardise64(a[:n], ddof, rm), standardise64(m[:n], ddof, rm)
    Kc = K if mistake == "window_not_clamped" else min(K, n - 1)
    if n <= DIRECT_MAX:
        full = np.correlate(ah, mh, "full")      # index n - 1 + k is lag k
    else:      # (a float64 FFT above that, for the time it saves: its error, 1e-12 here, is covered by the 1e-9 (1 + |c|) of radii())
        from scipy.signal import correlate
        full = correlate(ah, mh, "full", method="fft")
    c = np.zeros(2 * Kc + 1)
    kk = np.arange(-Kc, Kc + 1)
    ok = np.abs(kk) <= n - 1
    c[ok] = full[n - 1 + kk[ok]]
    return {"n": n, "Kc": Kc, "c": c, "a_std": ah, "m_std": mh}


def lag64(a, m, sr: float = 16000.0, fps: float = 25.0, max_lag_s: float = 0.5, mistake: str = None) -> float:
    """The seconds the restatement returns; `mistake`: one of MISTAKES (the table that shows the checks are not vacuous)."""
    assert mistake is None or mistake in MISTAKES, mistake
    K = int(max_lag_s * (fps if mistake == "k_from_fps" else sr))
    w = window64(a, m, K, mistake)
    if w is None:
        return 0.0
    c = w["c"]
    j = int(c.size - 1 - np.argmax(c[::-1])) if mistake == "ties_highest" else int(np.argmax(c))
    k = j - w["Kc"] + int(mistake == "centre_off_by_one")
    return float((-k if mistake == "sign_flipped" else k) / sr)


def margin(c: np.ndarray) -> float:
    """The lead of the largest value over the runner-up (inf for a window of one lag)."""
    if c.size < 2:
        return float("inf")
    top = np.sort(c)[-2:]
    return float(top[1] - top[0])


# ----------------------------------------------------------------------------------------------------------------- the exact mirror
def _block_sum(v: np.ndarray) -> float:
    """Thread t adds v[t], v[t + 1024], ... in ascending order (double); the 1024 partials fold by halves."""
    rows = -(-v.size // ROW_THREADS)
    p = np.zeros(rows * ROW_THREADS)
    p[:v.size] = v
    p = p.reshape(rows, ROW_THREADS)
    red = np.zeros(ROW_THREADS)
    for r in range(rows):      # (adding the +0.0 of the padding changes no value)
        red = red + p[r]
    o = ROW_THREADS // 2
    while o:
        red[:o] = red[:o] + red[o:2 * o]
        o //= 2
    return float(red[0])


def standardise32(x) -> np.ndarray:
    """The device's standardised row of x (all of it: pass x[:n]), every bit."""
    x = _f32(x)
    n = x.size
    xd = x.astype(np.float64)
    mean = _block_sum(xd) / float(n)
    d = xd - mean
    var = _block_sum(d * d) / float(n)
    mean32, den = np.float32(mean), np.float32(np.float32(np.sqrt(var)) + np.float32(1e-9))
    return ((x - mean32) / den).astype(np.float32)


def corr32(ah32: np.ndarray, mh32: np.ndarray, K: int) -> np.ndarray:
    """The device's c[-Kc .. Kc] from ITS standardised rows, every bit."""
    n = ah32.size
    Kc = min(K, n - 1)
    ap = np.zeros(n + 2 * Kc, dtype=np.float32)      # ap[Kc + g] = ahat[g]
    ap[Kc:Kc + n] = ah32
    c = None
    for s0 in range(0, n, SEG):
        acc = np.zeros(2 * Kc + 1, dtype=np.float32)
        for i in range(s0, min(s0 + SEG, n)):
            acc = fma32(ap[i:i + 2 * Kc + 1], mh32[i], acc)      # column j is lag j - Kc: ahat[i + j - Kc]
        c = acc if c is None else (c + acc).astype(np.float32)
    return (c + np.float32(0.0)).astype(np.float32)


def mirror(a, m, K: int) -> dict:
    """{"n", "Kc", "a_std", "m_std", "c", "lag", "peak"} as the device computes them, every bit; None for n < 4."""
    a, m = _f32(a), _f32(m)
    n = min(a.size, m.size)
    if n < 4:
        return None
    ah, mh = standardise32(a[:n]), standardise32(m[:n])
    c = corr32(ah, mh, K)
    j = int(np.argmax(c))
    return {"n": n, "Kc": min(K, n - 1), "a_std": ah, "m_std": mh, "c": c, "lag": j - min(K, n - 1), "peak": np.float32(c[j] / np.float32(n))}


# ----------------------------------------------------------------------------------------------------------------- the radii
def std_radius(x) -> np.ndarray:
    """|device xhat_i - float64 xhat_i| <= this, per sample (module docstring)."""
    x = _f32(x).astype(np.float64)
    n = x.size
    mu = x.mean()
    N = x - mu
    sigma = np.sqrt((N * N).sum() / n)
    D = sigma + 1e-9
    d = n * 2.0 ** -52 * np.abs(x).max()
    e_mu = U * abs(mu) + 2.0 * d
    e_N = e_mu + U * (np.abs(N) + e_mu)
    e_s = U * sigma + 2.0 * n * 2.0 ** -52 * sigma
    e_D = e_s + U * 1e-9 + U * (D + e_s)
    q = e_N / (D - e_D) + np.abs(N) * e_D / (D * (D - e_D))
    return q + U * (np.abs(N) / D + q)


def _window_fft(a: np.ndarray, m: np.ndarray, Kc: int) -> np.ndarray:
    """sum_i a[i + k] m[i], k = -Kc .. Kc, of non-negative series by a float64 FFT, widened by the FFT's own error."""
    from scipy.signal import correlate
    n = a.size
    full = np.maximum(correlate(a, m, "full", method="fft"), 0.0)
    w = full[n - 1 - Kc:n + Kc]
    return w + 1e-9 * (1.0 + w)


def radii(a, m, K: int) -> dict:
    """{"a_std", "m_std": per sample, "c": per lag of -Kc .. Kc, "peak": per lag} around window64(a, m, K); None for n < 4."""
    w = window64(a, m, K)
    if w is None:
        return None
    n, Kc = w["n"], w["Kc"]
    ea, em = std_radius(_f32(a)[:n]), std_radius(_f32(m)[:n])
    A, M = np.abs(w["a_std"]), np.abs(w["m_std"])
    L = min(n, SEG) + (-(-n // SEG) - 1) + 1
    g = L * U / (1.0 - L * U)
    rc = g * _window_fft(A + ea, M + em, Kc) + _window_fft(ea, M, Kc) + _window_fft(A, em, Kc) + _window_fft(ea, em, Kc)
    rc = rc + 1e-9 * (1.0 + np.abs(w["c"]))      # (window64 above DIRECT_MAX samples)
    rp = rc / n + U * (np.abs(w["c"]) + rc) / n
    return {"a_std": ea, "m_std": em, "c": rc, "peak": rp}


def possible_lags(c64: np.ndarray, rc: np.ndarray, Kc: int) -> np.ndarray:
    """The lags an arithmetic within the radii may choose: {k : c[k] >= max c - 2 max radius}."""
    return np.flatnonzero(c64 >= c64.max() - 2.0 * rc.max()) - Kc


# ----------------------------------------------------------------------------------------------------------------- the fixture
def load_fixture(path) -> dict:
    """name -> {"a", "m", "sr", "fps", "max_lag_s", "seconds", "shift", "kind"} from tests/golden/avlag.npz."""
    z = np.load(path)
    out = {}
    for name in z["names"]:
        name = str(name)
        out[name] = {"a": z[f"{name}/a"], "m": z[f"{name}/m"], "sr": float(z[f"{name}/sr"]), "fps": float(z[f"{name}/fps"]),
                     "max_lag_s": float(z[f"{name}/max_lag_s"]), "seconds": float(z[f"{name}/seconds"]), "shift": int(z[f"{name}/shift"]),
                     "kind": str(z[f"{name}/kind"])}
    return out
