"""Cases, float64 references, derived per-element bounds, float32 restatements and mutants of the audio encoder's own kernels
(csrc/audio.hip): ufnd_w2v2_frames, ufnd_w2v2_pos_pack, ufnd_w2v2_pos_add, ufnd_wave_normalize, ufnd_w2v2_conv0, and the positional
conv assembled from pack -> 16 ufnd_conv1d_rows_bf16 launches -> add.  Shared by tests/test_audio_ops_cases.py (CPU: every
restatement stays inside its bound, every mutant leaves it by MUTANT_FACTOR or breaks an equality) and tests/test_gpu_audio_ops.py
(GPU: every case through the C ABI).  The layout is tests/frozen_ops_cases.py's: Op(cases, make, reference, restate, mutants),
worst_ratio, a bound of 0 = bit equality.  The overlapping-row GEMM itself has its table in tests/conv_rows_cases.py.

THE TWO STATISTICS KERNELS.  u = 2^-24.  With mu and v the mean and the population variance of the fp32 values in float64, c = x - mu,
r = 1 / sqrt(v + eps), and d the depth of the kernel's sums (ufnd_wave_normalize: 16 sequential additions per thread and 8 tree levels,
d = 24; ufnd_w2v2_conv0: 64 and 2, d = 66):
    d_mu  = u |mu| + (d + 1) u a + mean(ex)        a = mean_i |x_i - m(i)|, m(i) the float64 mean of i's chunk (4,096 samples / 256 frames)
    d_v   = (d + 4) u v + 2 d_mu mean|c| + d_mu^2 + 2 mean(|c| ex) + mean(ex^2)
    d_r   = r (d_v / (2 (v + eps)) + 2 u)
    bound = r (d_mu + ex + u |c|) + |c| d_r + u |out|
ex is the bound the values already carry (0 for samples; the conv's fma chain for ufnd_w2v2_conv0's frames).
Where the term `a` comes from: a chunk's partial is a sum of fl(x_i - centre), each rounded once and added at depth d: (d + 1) u
sum_i |x_i - centre|; the chunks' means are then combined in float64.  With the centre AT the chunk's own mean (to within a few fp32
ulps of the values, which is second order: ufnd_wave_normalize takes a first pass for it, ufnd_w2v2_conv0 the conv of the chunk's mean
window) that is (d + 1) u a, and a <= 2 mean|c| by the triangle inequality (a = mean|c| where the chunk
means agree).  A centre that is NOT the chunk's mean -- the chunk's first value, say, when that value is a click -- has no such bound:
NO TERM HERE CONTAINS A PIVOT OR ITS DISTANCE FROM THE MEAN, so a kernel whose accuracy depends on where in a chunk an outlier sits
leaves the bound; the "pivot_sensitive" mutant (sums about the chunk's first value, m2 = q - s^2 / n in float64) is that kernel.
No term comes from a kernel's output.

A constant clip must come out as exact zeros (ufnd_wave_normalize) / as one value per channel, gelu_fast(beta) (ufnd_w2v2_conv0): the
mean, rounded to fp32, IS the value, and every difference from it is 0 exactly."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

from tests import conv_rows_cases as CR
from tests import gemm_bf16_cases as G
from tests.frozen_ops_cases import HW_ULP, Op, U, bf16_bits, bf16_f32, bf16_round, worst_ratio  # noqa: F401

MUTANT_FACTOR = 4.0
SENT_F32 = np.float32(12345.678)
SENT_BF16 = np.uint16(0x4E4E)
SENT_I32 = np.int32(-77)
NAN_BF16 = np.uint16(0x7FC0)
TAIL = 2                           # sentinel rows behind every output
WCH, FCH = 4096, 256               # UFND_WAVE_CHUNK, UFND_CONV0_CHUNK
HID, POS_G, POS_C, POS_K = 768, 16, 48, 128
C0 = 512
f32 = np.float32


def _seed(*ints) -> np.random.Generator:
    return np.random.default_rng([20240] + [int(i) for i in ints])


def _bits_ref(bits):
    """a buffer of bit patterns as a (reference, bound 0) pair"""
    b = np.asarray(bits).astype(np.float64)
    return b, np.zeros_like(b)


# ------------------------------------------------------------------ ufnd_w2v2_frames (exact)
FRAME_LENGTHS = list(range(400, 2101)) + [16000, 41360, 41680, 480000, 2 ** 24 + 7]
_LAYERS = ((10, 5), (3, 2), (3, 2), (3, 2), (3, 2), (2, 2), (2, 2))


def hf_frames(n: int) -> int:
    """transformers' _get_feat_extract_output_lengths: floor((t - k) / s) + 1 per layer, in Python integers"""
    t = int(n)
    for k, s in _LAYERS:
        t = (t - k) // s + 1
    return t


def _frames_cases():
    return [("all", 1), ("all", 2), ("all", 131), ("30s", 1500)]


def _frames_make(case):
    which, _ = case
    return dict(lengths=np.array(FRAME_LENGTHS if which == "all" else [480000, 400, 479999], dtype=np.int32))


def _frames_reference(case, inp):
    S = case[1]
    T = np.array([hf_frames(n) for n in inp["lengths"].tolist()], dtype=np.int64)
    return {"frames": _bits_ref(T), "key_mask": _bits_ref(np.arange(S)[None, :] < T[:, None])}


def _frames_restate(case, inp, mutant=None):
    S = case[1]
    t = inp["lengths"].astype(np.int64)
    for i, (k, s) in enumerate(_LAYERS):      # vectorised int64 arithmetic, the quotient through divmod
        q, rem = np.divmod(t - k, s)
        t = q + 1 + ((rem != 0) if (mutant == "one_floor_is_a_ceiling" and i == 4) else 0)
    mask = np.arange(S)[None, :] <= t[:, None] if mutant == "t_le_T" else np.arange(S)[None, :] < t[:, None]
    return {"frames": t.astype(np.int32), "key_mask": mask.astype(np.int32)}


# ------------------------------------------------------------------ ufnd_w2v2_pos_pack / ufnd_w2v2_pos_add
POS_SHAPES = [(1, 1, (1,)), (3, 5, (1, 5, 3)), (2, 131, (130, 64))]


def _pack_make(case):
    B, S, frames = case
    rng = _seed(1, B, S)
    x = bf16_bits(rng.standard_normal((B * S, HID)).astype(f32))
    for b in range(B):
        x[b * S + frames[b]:(b + 1) * S] = NAN_BF16      # a slab's rows past frames[b]: zeros must come out, not copies
    return dict(x=x, frames=np.array(frames, dtype=np.int32))


def pack_rows(x: np.ndarray, frames, B: int, S: int, mutant=None, fill=np.uint16(0)) -> np.ndarray:
    """(16, Mp, 48) bf16 bits: include/ultrafnd_hip.h's layout, written out row by row"""
    Sp, off = S + POS_K, 63 if mutant == "offset_63" else POS_K // 2
    Mp = B * Sp + POS_K
    out = np.zeros((POS_G, Mp, POS_C), np.uint16)
    if mutant == "spare_rows_left_unwritten":
        out[:, B * Sp:] = fill
    for b in range(B):
        for t in range(min(int(frames[b]), S)):
            row = off + b * S + t if mutant == "padding_at_the_batch_edges" else b * Sp + off + t
            out[:, row] = x[b * S + t].reshape(POS_G, POS_C)
    return out


def _pack_reference(case, inp):
    B, S, _ = case
    return {"packed": _bits_ref(pack_rows(inp["x"], inp["frames"], B, S))}


def _pack_restate(case, inp, mutant=None):
    """index arithmetic instead of the row loop: every element of `packed` names its source"""
    B, S, _ = case
    if mutant is not None:
        return {"packed": pack_rows(inp["x"], inp["frames"], B, S, mutant, fill=SENT_BF16)}
    Sp = S + POS_K
    Mp = B * Sp + POS_K
    prow = np.arange(Mp)
    b, t = prow // Sp, prow % Sp - POS_K // 2
    bc = np.minimum(b, B - 1)
    live = (b < B) & (t >= 0) & (t < S) & (t < inp["frames"][bc])
    src = np.where(live, bc * S + t, 0)
    rows = np.where(live[:, None], inp["x"][src], np.uint16(0))                 # (Mp, 768)
    return {"packed": np.ascontiguousarray(rows.reshape(Mp, POS_G, POS_C).transpose(1, 0, 2))}


def _add_make(case):
    B, S, frames = case
    rng = _seed(2, B, S)
    Sp = S + POS_K
    x = rng.standard_normal((B * S, HID)).astype(f32)
    conv = np.full((POS_G, B * Sp, 64), np.nan, f32)      # rows past frames[b] (the slab tail and the 128 pad rows) are never read
    for b in range(B):
        x[b * S + frames[b]:(b + 1) * S] = np.nan
        conv[:, b * Sp:b * Sp + frames[b]] = rng.standard_normal((POS_G, frames[b], 64)).astype(f32)      # columns 48 .. 63 hold values too
    return dict(x=x, conv=conv, frames=np.array(frames, dtype=np.int32))


def add_rows(x, conv, frames, B, S, dtype, mutant=None):
    Sp = S + POS_K
    y = np.zeros((B * S, HID), dtype)
    flat = conv.reshape(-1, 64)
    for b in range(B):
        for t in range(int(frames[b])):
            for g in range(POS_G):
                row = g * B * S + b * Sp + t if mutant == "group_stride_B_S" else g * B * Sp + b * Sp + t
                cols = np.arange(POS_C)
                if mutant == "columns_48_63_of_the_panel_read":      # 16 pieces of 4 per group instead of 12
                    p = g * 12 + cols // 4
                    row, cols = (p // 16) * B * Sp + b * Sp + t, (p % 16) * 4 + cols % 4
                cv = flat[np.minimum(row, flat.shape[0] - 1), cols]
                y[b * S + t, POS_C * g:POS_C * (g + 1)] = x[b * S + t, POS_C * g:POS_C * (g + 1)].astype(dtype) + cv.astype(dtype)
    return y


def _add_reference(case, inp):
    """one fp32 addition is correctly rounded: the float64 sum of two fp32 values, rounded once, IS the result (bound 0 on the bits'
    values; the rows past frames[b] are +0)"""
    B, S, _ = case
    y = add_rows(inp["x"], inp["conv"], inp["frames"], B, S, np.float64).astype(f32).astype(np.float64)
    return {"y": (y, np.zeros_like(y))}


def _add_restate(case, inp, mutant=None):
    B, S, _ = case
    with np.errstate(invalid="ignore"):
        return {"y": add_rows(inp["x"], inp["conv"], inp["frames"], B, S, f32, mutant)}


# ------------------------------------------------------------------ the chunked statistics of both kernels, in float32
def _tree(a):
    """pairwise levels over axis 0 (a power of two)"""
    while a.shape[0] > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def chunk_stats32(y: np.ndarray, chunk: int, width: int, how: str = "recentred", count_full: bool = False, centre_of=None):
    """float64 (mean, M2) per column of the fp32 values y (n, C) the way the kernels form them: per chunk, `width` threads each add
    their values (i = thread, thread + width, ...) in sequence, a pairwise tree joins the threads, and the chunks' {centre, s, q} are
    combined in chunk order in float64 (Chan).  how = "recentred": the sums run about the chunk's own fp32 mean -- centre_of(c0, c1)
    where the caller has its own way to it (ufnd_w2v2_conv0: the conv of the chunk's mean window), otherwise a first pass about the
    chunk's first value (ufnd_wave_normalize); "pivot": about the chunk's first value (the pivot-sensitive arithmetic)."""
    n, C = y.shape
    n_a, mean_a, m2_a = 0.0, np.zeros(C), np.zeros(C)

    def sums(d):
        pad = np.zeros((chunk - d.shape[0], C), f32)
        d = np.concatenate([d, pad]).reshape(chunk // width, width, C)
        s, q = np.zeros((width, C), f32), np.zeros((width, C), f32)
        for j in range(d.shape[0]):
            s = s + d[j]
            q = q + d[j] * d[j]
        return _tree(s), _tree(q)
    for c0 in range(0, n, chunk):
        seg = y[c0:c0 + chunk]
        cnt = chunk if count_full else seg.shape[0]
        centre = seg[0]
        s, q = sums(seg - centre)
        if how == "recentred":
            centre = centre + s / f32(seg.shape[0]) if centre_of is None else centre_of(c0, c0 + seg.shape[0])
            s, q = sums(seg - centre)
        n_b = float(cnt)
        mean_b = centre.astype(np.float64) + s.astype(np.float64) / n_b
        m2_b = np.maximum(q.astype(np.float64) - s.astype(np.float64) ** 2 / n_b, 0.0)
        n_ab, delta = n_a + n_b, mean_b - mean_a
        mean_a = mean_a + delta * (n_b / n_ab)
        m2_a = m2_a + m2_b + delta * delta * (n_a * n_b / n_ab)
        n_a = n_ab
    return mean_a, m2_a


def stats_bound(x64: np.ndarray, ex, eps: float, chunk: int, d: int):
    """(mu, r, c, d_mu, d_r) of the columns of x64 (n, C) by the module docstring's formulas"""
    n = x64.shape[0]
    mu = x64.mean(0)
    c = x64 - mu
    v = (c * c).mean(0)
    r = 1.0 / np.sqrt(v + eps)
    a = np.concatenate([np.abs(x64[i:i + chunk] - x64[i:i + chunk].mean(0)) for i in range(0, n, chunk)]).mean(0)
    ex = np.broadcast_to(ex, x64.shape)
    mc = np.abs(c).mean(0)
    d_mu = U * np.abs(mu) + (d + 1) * U * a + ex.mean(0)
    d_v = (d + 4) * U * v + 2 * d_mu * mc + d_mu ** 2 + 2 * (np.abs(c) * ex).mean(0) + (ex * ex).mean(0)
    d_r = r * (d_v / (2 * (v + eps)) + 2 * U)
    return mu, r, c, d_mu, d_r


STAT_MUTANTS = ("last_chunk_counted_as_full", "unbiased_variance", "pivot_sensitive")

# ------------------------------------------------------------------ ufnd_wave_normalize
WAVE_LENGTHS = (400, 4095, 4096, 4097, 8192, 8193, 12289)
WAVE_BATCH = (4097, 12289, 400)            # one ragged launch; every row must equal the clip alone bit for bit
WAVE_N = 9999                              # the length of the data-kind clips: chunks of 4,096 + 4,096 + 1,807
WAVE_KINDS = ("dc_heavy", "click20_at_4096", "click100_at_4096", "click20_at_0", "click100_at_0", "click20_at_4097", "click100_at_4097",
              "constant", "constant_but_the_last")
WAVE_EPS = 1e-7
WAVE_D = 24


def is_chunk_start_click(kind: str) -> bool:
    """the clips on which the pivot-sensitive arithmetic must leave the bound: a click that IS a chunk's first sample"""
    return kind.startswith("click") and int(kind.rsplit("_", 1)[1]) % WCH == 0


def smooth_wave(n: int) -> np.ndarray:
    from tests import audio_ref            # (imports torch; only the smooth clips need it)
    return audio_ref.make_waves([n], seed=n)[0].numpy()


def wave_clip(kind: str, n: int) -> np.ndarray:
    if kind == "smooth":
        return smooth_wave(n)
    rng = _seed(3, n, WAVE_KINDS.index(kind))
    noise = rng.standard_normal(n)
    if kind == "dc_heavy":
        return (0.9 + 0.001 * noise).astype(f32)
    if kind == "constant":
        return np.full(n, 0.0371, f32)
    if kind == "constant_but_the_last":
        x = np.full(n, 0.0371, f32)
        x[-1] = f32(0.05)
        return x
    x = 0.05 * noise + 0.02
    sig, at = kind[len("click"):].split("_at_")
    x[int(at)] = 0.02 + float(sig) * 0.05
    return x.astype(f32)


def _wave_cases():
    return [("smooth", (n,)) for n in WAVE_LENGTHS] + [("smooth", WAVE_BATCH)] + [(k, (WAVE_N,)) for k in WAVE_KINDS]


def _wave_make(case):
    kind, lengths = case
    n_max = max(lengths)
    wave = np.full((len(lengths), n_max), np.nan, f32)      # NaN past each length: never read
    for b, n in enumerate(lengths):
        wave[b, :n] = wave_clip(kind, n)
    return dict(wave=wave, lengths=np.array(lengths, dtype=np.int32))


def _wave_reference(case, inp):
    """per clip "out{b}": (float64 normalisation of the fp32 samples, bound); the constant clip: exact zeros"""
    kind, lengths = case
    out = {}
    for b, n in enumerate(lengths):
        x = inp["wave"][b, :n].astype(np.float64)[:, None]
        mu, r, c, d_mu, d_r = stats_bound(x, 0.0, WAVE_EPS, WCH, WAVE_D)
        ref = c * r
        bound = r * (d_mu + U * np.abs(c)) + np.abs(c) * d_r + U * np.abs(ref)
        if kind == "constant":      # (the float64 mean of n equal values is that value up to its own rounding: the result IS 0)
            assert np.abs(c).max() <= 1e-12 * abs(mu[0])
            ref, bound = np.zeros_like(ref), np.zeros_like(ref)
        out[f"out{b}"] = (ref[:, 0], bound[:, 0])
    return out


def _wave_restate(case, inp, mutant=None):
    _, lengths = case
    out = {}
    for b, n in enumerate(lengths):
        x = inp["wave"][b, :n]
        mean, m2 = chunk_stats32(x[:, None], WCH, 256, "pivot" if mutant == "pivot_sensitive" else "recentred",
                                 count_full=mutant == "last_chunk_counted_as_full")
        var = m2[0] / ((n - 1) if mutant == "unbiased_variance" else n)
        out[f"out{b}"] = (x - f32(mean[0])) * f32(1.0 / math.sqrt(var + WAVE_EPS))
    return out


# ------------------------------------------------------------------ ufnd_w2v2_conv0
CONV0_LENGTHS = (400, 645, 1284, 1285, 1290, 2570)          # T1 = 79, 128, 255, 256, 257, 513
CONV0_BATCH = (1285, 2570, 400)
CONV0_N = 2570                                                # the data-kind clips: frame chunks of 256 + 256 + 1
CONV0_KINDS = ("click10_in_frame_256", "click100_in_frame_256", "click10_one_frame_later", "click100_one_frame_later", "channel_x20", "constant")
CONV0_EPS = 1e-5
CONV0_D = 66
CONV0_SCALED_CHANNEL = 5


def conv0_T1(n: int) -> int:
    return (n - 10) // 5 + 1


def conv0_S1(lengths, extra: int) -> int:
    return -(-conv0_T1(max(lengths)) // 64) * 64 + extra


def is_chunk_start_frame_click(kind: str) -> bool:
    return kind.endswith("_in_frame_256")


def conv0_clip(kind: str, n: int) -> np.ndarray:
    """clips as ufnd_w2v2_conv0 sees them: normalised (mean 0, variance 1)"""
    if kind in ("smooth", "channel_x20"):
        x = smooth_wave(n).astype(np.float64)
        return ((x - x.mean()) / np.sqrt(x.var() + 1e-7)).astype(f32)
    if kind == "constant":
        return np.full(n, 0.4321, f32)
    x = _seed(4, n, CONV0_KINDS.index(kind)).standard_normal(n)
    sig = float(kind[len("click"):].split("_")[0])
    # frame t reads samples 5 t .. 5 t + 9.  Sample 1287 lies in frames 256 (the second chunk's first frame) and 257 only; sample
    # 1292, one frame later, in frames 257 and 258
    x[1287 if is_chunk_start_frame_click(kind) else 1292] = sig
    return x.astype(f32)


def _conv0_cases():
    out = [("smooth", (n,), extra) for n in CONV0_LENGTHS for extra in (0, 64)]
    out += [("smooth", CONV0_BATCH, 0), ("smooth", CONV0_BATCH, 64)]
    return out + [(k, (CONV0_N,), 0) for k in CONV0_KINDS]


def _conv0_make(case):
    kind, lengths, extra = case
    rng = _seed(5)
    n_max = max(lengths)
    wave = np.full((len(lengths), n_max), np.nan, f32)
    for b, n in enumerate(lengths):
        wave[b, :n] = conv0_clip(kind, n)
    w = (rng.standard_normal((C0, 10)) * math.sqrt(2.0 / 10)).astype(f32)
    if kind == "channel_x20":
        w[CONV0_SCALED_CHANNEL] *= f32(20)
    return dict(wave=wave, lengths=np.array(lengths, dtype=np.int32), w=w, gamma=(1.0 + 0.1 * rng.standard_normal(C0)).astype(f32),
                beta=(0.05 * rng.standard_normal(C0)).astype(f32))


def _frames_of(x, T1):
    return x[(5 * np.arange(T1))[:, None] + np.arange(10)[None, :]]      # (T1, 10)


def _conv0_reference(case, inp):
    """per clip "of{b}" / "ob{b}" (T1, 512): (GELU(GroupNorm(conv)) in float64, bound).  y = sum_k w_k x_k is a 10-term fma chain:
    ex = 10 u sum |w x|; the statistics per channel over the clip's T1 frames (module docstring, d = 66); n0 = fl(fl(y - mean) rstd):
    e1 = r (d_mu + ex + u |c|) + |c| d_r + u |n0|; a = fma(n0, gamma, beta): e2 = |gamma| e1 + u |a|; gelu_fast against the exact
    erf-GELU: gemm_bf16_cases' terms (slope 1.13, ACT_ABS, ACT_HW |a|, u |out|).  ACT_ABS was measured over |a| <= 10; beyond it
    erf's tail is below 1e-22 and gelu_fast is fl(h + h) or fl(h - h), exact: the terms hold there too.  "ob" takes the same pair
    (judged by the bf16 interval rule)."""
    kind, lengths, _ = case
    w = inp["w"].astype(np.float64)
    gm, bt = inp["gamma"].astype(np.float64), inp["beta"].astype(np.float64)
    out = {}
    for b, n in enumerate(lengths):
        T1 = conv0_T1(n)
        xf = _frames_of(inp["wave"][b, :n].astype(np.float64), T1)
        y = xf @ w.T
        ex = 10 * U * (np.abs(xf) @ np.abs(w).T)
        mu, r, c, d_mu, d_r = stats_bound(y, ex, CONV0_EPS, FCH, CONV0_D)
        n0 = c * r
        e1 = r * (d_mu + ex + U * np.abs(c)) + np.abs(c) * d_r + U * np.abs(n0)
        a = n0 * gm + bt
        e2 = np.abs(gm) * e1 + U * np.abs(a)
        if kind == "constant":      # every difference y - mean is 0 exactly: nothing but the activation's own terms
            assert np.abs(c).max() <= 1e-12 * np.abs(mu).max()
            a, e2 = np.broadcast_to(bt, a.shape).copy(), np.zeros_like(a)
        ref = G.act64(G.ACT_GELU, a)
        bound = G.ACT_SLOPE * e2 + G.measure_act_errors()[G.ACT_GELU] + G.ACT_HW[G.ACT_GELU] * np.abs(a) + U * np.abs(ref)
        out[f"of{b}"] = (ref, bound)
        out[f"ob{b}"] = (ref, bound)
    return out


def _conv0_restate(case, inp, mutant=None):
    _, lengths, _ = case
    out = {}
    for b, n in enumerate(lengths):
        T1 = conv0_T1(n)
        xf = _frames_of(inp["wave"][b, :n], T1)
        y = np.zeros((T1, C0), f32)
        for k in range(10):
            y = G._fma(inp["w"][None, :, k], xf[:, k:k + 1], y)
        w = inp["w"]

        def mean_window_conv(t0, t1):      # the conv is linear: its mean over the frames is the conv of the ten sample means
            xm = _tree(np.concatenate([xf[t0:t1], np.zeros((FCH - (t1 - t0), 10), f32)])) / f32(t1 - t0)
            c = np.zeros(C0, f32)
            for k in range(10):
                c = G._fma(w[:, k], xm[k], c)
            return c
        mean, m2 = chunk_stats32(y, FCH, 4, "pivot" if mutant == "pivot_sensitive" else "recentred", count_full=mutant == "last_chunk_counted_as_full",
                                 centre_of=mean_window_conv)
        var = m2 / ((T1 - 1) if mutant == "unbiased_variance" else T1)
        v = G.gelu_fast_f32(G._fma((y - mean.astype(f32)) * (1.0 / np.sqrt(var + CONV0_EPS)).astype(f32), inp["gamma"], inp["beta"]))
        out[f"of{b}"] = v
        out[f"ob{b}"] = bf16_round(v)
    return out


# ------------------------------------------------------------------ the positional conv, assembled
POSCONV_CASE = (4, 66, (1, 3, 64, 65))


def _posconv_make(case):
    """x0 (B S, 768) fp32 and its bf16 rounding (rows past frames[b] NaN), the encoder's own parametrisation resolved and grouped"""
    import torch
    from ultrafnd_git_amd.audio import pos_group_weights, resolve_weight_norm
    B, S, frames = case
    rng = _seed(6)
    x = rng.standard_normal((B * S, HID)).astype(f32)
    for b in range(B):
        x[b * S + frames[b]:(b + 1) * S] = np.nan
    v = torch.from_numpy((rng.standard_normal((HID, POS_C, POS_K)) * 2.0 * math.sqrt(1.0 / (POS_K * HID))).astype(f32))
    g = v.norm(p=2, dim=(0, 1), keepdim=True) * torch.from_numpy((1.0 + 0.1 * rng.standard_normal((1, 1, POS_K))).astype(f32))
    w = resolve_weight_norm(g, v)                                               # (768, 48, 128) fp32, as the encoder resolves it
    bias = torch.from_numpy((0.05 * rng.standard_normal(HID)).astype(f32))
    wg, bg = pos_group_weights(w, bias)
    return dict(x=x, xb=bf16_bits(x), frames=np.array(frames, dtype=np.int32), w=bf16_bits(w.numpy()), bias=bias.numpy(), wg=bf16_bits(wg.numpy()),
                bg=bg.numpy())


def _posconv_windows(inp, B, S, dtype):
    """per clip and group the (frames, 128 x 48) zero-padded tap windows of the bf16-rounded rows, and the tap-major weights"""
    xb = bf16_f32(inp["xb"]).astype(dtype)
    wt = bf16_f32(inp["w"]).astype(dtype).reshape(POS_G, POS_C, POS_C, POS_K).transpose(0, 1, 3, 2).reshape(POS_G, POS_C, POS_K * POS_C)
    for b in range(B):
        T = int(inp["frames"][b])
        pad = np.zeros((T + POS_K, HID), dtype)
        pad[POS_K // 2:POS_K // 2 + T] = xb[b * S:b * S + T]
        for g in range(POS_G):
            rows = pad[:, POS_C * g:POS_C * (g + 1)]
            win = rows[np.arange(T)[:, None] + np.arange(POS_K)[None, :]].reshape(T, POS_K * POS_C)      # conv1d(padding=64)[..., :-1]
            yield b, g, T, win, wt[g]


def _posconv_reference(case, inp):
    """y = x + GELU(conv + bias): the conv a float64 grouped conv1d(padding = 64)[..., :-1] over each clip's own frames on the
    bf16-rounded operands; the bound is conv_rows_cases' per-element GEMM bound (K = 6,144) through the GELU plus one fp32 addition,
    u |y|.  Rows past frames[b] are exact zeros."""
    B, S, _ = case
    ref, bound = np.zeros((B * S, HID)), np.zeros((B * S, HID))
    for b, g, T, win, wt in _posconv_windows(inp, B, S, np.float64):
        acc = win @ wt.T
        e = G.ACC_ULP * POS_K * POS_C * (np.abs(win) @ np.abs(wt).T)
        v, e = CR.epilogue_ref(acc, e, inp["bias"][POS_C * g:POS_C * (g + 1)].astype(np.float64), G.ACT_GELU, False)
        sl = (slice(b * S, b * S + T), slice(POS_C * g, POS_C * (g + 1)))
        ref[sl] = inp["x"][sl].astype(np.float64) + v
        bound[sl] = e + U * np.abs(ref[sl])
    return {"y": (ref, bound)}


def _posconv_restate(case, inp, mutant=None):
    B, S, _ = case
    y = np.zeros((B * S, HID), f32)
    for b, g, T, win, wt in _posconv_windows(inp, B, S, f32):
        acc = (win @ wt.T).astype(f32) + inp["bias"][POS_C * g:POS_C * (g + 1)]
        sl = (slice(b * S, b * S + T), slice(POS_C * g, POS_C * (g + 1)))
        y[sl] = inp["x"][sl] + G.gelu_fast_f32(acc)
    return {"y": y}


OPS: Dict[str, Op] = {
    "w2v2_frames": Op(_frames_cases(), _frames_make, _frames_reference, _frames_restate, ("one_floor_is_a_ceiling", "t_le_T")),
    "w2v2_pos_pack": Op(POS_SHAPES, _pack_make, _pack_reference, _pack_restate, ("padding_at_the_batch_edges", "offset_63", "spare_rows_left_unwritten")),
    "w2v2_pos_add": Op(POS_SHAPES, _add_make, _add_reference, _add_restate, ("group_stride_B_S", "columns_48_63_of_the_panel_read")),
    "w2v2_pos_conv": Op([POSCONV_CASE], _posconv_make, _posconv_reference, _posconv_restate),
    "wave_normalize": Op(_wave_cases(), _wave_make, _wave_reference, _wave_restate, STAT_MUTANTS),
    "w2v2_conv0": Op(_conv0_cases(), _conv0_make, _conv0_reference, _conv0_restate, STAT_MUTANTS),
}


def case_id(case) -> str:
    def s(v):
        return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)
    return "-".join(s(v) for v in case)


def check(op: str, case, inp, got: Dict[str, np.ndarray], refs=None) -> Dict[str, float]:
    """error / bound of every output of a case: bf16 outputs ("ob..") by the interval rule of gemm_bf16_cases.bf16_ratio, everything
    else by worst_ratio; where the reference is an exact +0 a -0 counts as unequal (pos_add's promise)"""
    refs = OPS[op].reference(case, inp) if refs is None else refs
    assert set(refs) == set(got), (op, case, sorted(refs), sorted(got))
    out = {}
    for k, (ref, bound) in refs.items():
        g = np.asarray(got[k])
        if k.startswith("ob"):
            out[k] = G.bf16_ratio(g.reshape(ref.shape), ref, bound)
            continue
        r = worst_ratio(g.reshape(ref.shape), ref, bound)
        if g.dtype == np.float32 and (np.signbit(g.reshape(ref.shape)) & (ref == 0) & (bound == 0) & ~np.signbit(ref)).any():
            r = math.inf
        out[k] = r
    if op == "w2v2_conv0" and case[0] == "constant":      # one value per channel, whatever the frame
        for k, g in got.items():
            if not (np.asarray(g) == np.asarray(g)[:1]).all():
                out[k] = math.inf
    return out
