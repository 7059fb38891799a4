"""Cases, float64 references, derived error bounds, float32 restatements and mutants of the frozen encoders' non-GEMM kernels
(csrc/encoders.hip, csrc/attention.hip, ufnd_cast_bf16, ufnd_act_bf16, ufnd_gather_rows).  Shared by
tests/test_frozen_ops_cases.py (CPU: every restatement stays inside its bound, every mutant leaves it by MUTANT_FACTOR, the
table reaches every kernel instance) and tests/test_gpu_frozen_ops.py (GPU: every case through the C ABI against float64).

An op is an `Op`: `cases`, `make(case) -> inputs`, `reference(case, inputs) -> {output: (ref float64, bound float64)}`,
`restate(case, inputs, mutant=None) -> {output: array}` and the names of its mutants.  A bound of 0 means bit equality
(compared on the values; a NaN must stay a NaN).  `worst_ratio` is the one comparison both suites use.

How the bounds are derived (each formula is repeated beside its code):
  u = 2^-24 is the relative error of one fp32 operation (24 significand bits: half an ulp is at most 2^-24 of the value), BF = 2^-8
  that of one rounding to bf16 (8 significand bits, the implicit one included: an ulp is 2^-7 of the binade's lower end and half
  of it up to 2^-8 of the value -- 1 + 2^-8 is an exact tie between 1 and 1 + 2^-7; 2^-9 would fail a correctly rounded result,
  and the restatements' bf16 outputs reach 0.99 of the 2^-8 term).  A sum of depth d contributes d u sum|terms|.  The wave-per-row kernels (NI = H / 256 in 1..4) let every lane add 4 NI values in sequence and
  then combine the 64 lanes in a 6-level butterfly: d = 4 NI + 6, not H.  The 256-thread row kernels (L2 norms) add
  ceil(D / 256) values per thread, 6 butterfly levels and 2 levels over the four waves: d = ceil(D / 256) + 8.  Divisions and
  square roots are IEEE (hipcc's default: the kernels' code shows the v_div_scale / v_div_fmas / v_div_fixup ladder), one u each.
  Hardware approximations: v_rsq_f32 (rsqrtf in ln_row) and v_exp_f32 (the attention's exp2) are 1 ulp = 2^-23 relative in
  AMD's CDNA ISA reference ("1ULP accuracy").  No term of any bound comes from a kernel's output.

LayerNorm at a constant row and eps = 1e-12 is left out on purpose: there var = 0 and rstd = 1e6, so the rounding of the mean
(u |mean|) is multiplied by 1e6 in ANY fp32 LayerNorm -- the bound formula below says the same (its first term is
|gamma| rstd dmean), it would only assert that 0.06 <= 0.06.

The pooled ops end in v / (|v| + 1e-9): a wrong divisor in front of it (L instead of the live count, Mx instead of the valid
count) cancels unless |v| is near 1e-9, so their tables hold samples of that size.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

U = 2.0 ** -24            # one fp32 operation, relative
BF = 2.0 ** -8            # one rounding to bf16, relative (half an ulp of an 8-bit significand)
HW_ULP = 2.0 ** -23       # v_rsq_f32 / v_exp_f32 / v_rcp_f32: 1 ulp (CDNA ISA reference)
MUTANT_FACTOR = 4.0       # a mutant must leave the bound by this factor on at least one case

# dispatch thresholds of the C entries (read by the coverage test from here only)
ATTN_SHORT_L = 64                 # ufnd_attention_bf16: L <= 64 -> the 2-wave form
PATCHIFY_FAST = (32, 7)           # ufnd_vit_patchify: (patch, patches per row) of the compile-time instance
NI_VALUES = (1, 2, 3, 4)          # NI_LAUNCH: H / 256
GATHER_MAX_ITEMS = 8              # UFND_GATHER_MAX_ITEMS
CAST_GRID_CAP = 4096 * 256 * 4    # elements one sweep of ufnd_cast_bf16's capped grid covers
ACT_GRID_CAP = 4096 * 256 * 8     # the same for ufnd_act_bf16
SENTINEL_F32 = 12345.678          # outputs are filled with these before a launch
SENTINEL_BF16 = 0x4E4E


class Op(NamedTuple):
    cases: List[tuple]
    make: Callable
    reference: Callable
    restate: Callable
    mutants: Tuple[str, ...] = ()


# ---------------------------------------------------------------------------------------------------------------------
# bf16 as uint16 bit patterns
def bf16_bits(x) -> np.ndarray:
    """float32 -> bf16 bits, round to nearest even; a NaN stays a NaN (quiet bit set)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)


def bf16_f32(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x) -> np.ndarray:
    return bf16_f32(bf16_bits(x))


def bf16_ulp(v) -> np.ndarray:
    """The spacing of bf16 at |v| (8 significand bits): 2^(floor(log2 |v|) - 7); 0 at 0."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, 2.0 ** (e - 7), 0.0)


def worst_ratio(got, ref, bound) -> float:
    """max |got - ref| / bound; where bound == 0 the values must be equal (inf if not); a NaN on one side only is inf."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    if (gn != rn).any():
        return math.inf
    ok = ~rn
    with np.errstate(invalid="ignore"):
        err = np.where(ok, np.abs(np.where(ok, got, 0.0) - np.where(ok, ref, 0.0)), 0.0)
    err = np.where(ok & np.isinf(ref) & (got == ref), 0.0, err)
    exact = bound == 0
    if (err[exact] != 0).any():
        return math.inf
    if exact.all():
        return 0.0
    return float(np.max(err[~exact] / bound[~exact]))


def _seed(*ints) -> np.random.Generator:
    return np.random.default_rng(list(ints))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm of float64 rows x (M, H), with a per-element bound on the error the rows already carry (ex: 0 for exact inputs)
def ln_ref_bound(x, gamma, beta, eps, ex=None):
    """ref = (x - mean) / sqrt(var + eps) gamma + beta and the bound of the wave-per-row kernel's fp32 result.
    With d = 4 NI + 6, c = x - mean, rstd = 1 / sqrt(var + eps), ex = the error of the inputs (elementwise bound):
      dmean = (d + 1) u mean|x| + mean(ex)                    sum of depth d, the division by H, the inputs' own error
      dc_k  = dmean + u |c_k| + ex_k                          the subtraction x_k - mean
      dvar  = dmean^2 + 2 mean(|c| ex) + mean(ex^2)           sum((c - dmean)^2) / H = var + dmean^2 EXACTLY (sum c = 0): the mean's
              + (d + 4) u (var + dmean^2)                     error enters squared; 2 u from c's rounding, u from the square, d u
                                                              from the sum, u from the division
      rho   = (dvar + u (var + eps)) / (2 (var + eps)) + 2^-23         rstd, relative: the addition of eps, v_rsq_f32 at 1 ulp
      |dy_k| <= |gamma_k| rstd dc_k + |c_k rstd gamma_k| (rho + 2 u) + u |y_k|      two products, one addition
    The first term is what grows with max|x| rstd |gamma| (rows with a large mean)."""
    x = np.asarray(x, dtype=np.float64)
    H = x.shape[-1]
    d = 4 * (H // 256) + 6
    ex = np.zeros_like(x) if ex is None else ex
    mean = x.mean(-1, keepdims=True)
    c = x - mean
    var = (c * c).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = c * rstd * gamma + beta
    dmean = (d + 1) * U * np.abs(x).mean(-1, keepdims=True) + ex.mean(-1, keepdims=True)
    dc = dmean + U * np.abs(c) + ex
    dvar = dmean ** 2 + 2 * (np.abs(c) * ex).mean(-1, keepdims=True) + (ex * ex).mean(-1, keepdims=True) + (d + 4) * U * (var + dmean ** 2)
    rho = (dvar + U * (var + eps)) / (2 * (var + eps)) + HW_ULP
    bound = np.abs(gamma) * rstd * dc + np.abs(c * rstd * gamma) * (rho + 2 * U) + U * np.abs(y)
    return y, bound


def with_bf16(ref, bound):
    """The bound of the same value rounded to bf16: the fp32 error, and half a bf16 ulp of the value that was rounded."""
    return ref, bound + BF * (np.abs(ref) + bound)


def ln_f32(x, gamma, beta, eps, mutant=None):
    """fp32 LayerNorm in NumPy's own (pairwise) summation order."""
    x = _f32(x)
    H = np.float32(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=np.float32) / H
    if mutant == "one_pass_variance":
        var = (x * x).sum(-1, keepdims=True, dtype=np.float32) / H - mean * mean
    elif mutant == "divide_by_h_minus_1":
        var = ((x - mean) ** 2).sum(-1, keepdims=True, dtype=np.float32) / (H - np.float32(1))
    else:
        var = ((x - mean) ** 2).sum(-1, keepdims=True, dtype=np.float32) / H
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    if mutant == "beta_before_gamma":
        return ((x - mean) * rstd + _f32(beta)) * _f32(gamma)
    return (x - mean) * rstd * _f32(gamma) + _f32(beta)


def _outs(kind, y32, f="of", b="ob"):
    out = {}
    if kind in ("both", "f32"):
        out[f] = y32
    if kind in ("both", "bf16"):
        out[b] = bf16_round(y32)
    return out


def _ref_outs(kind, ref, bound, f="of", b="ob"):
    out = {}
    if kind in ("both", "f32"):
        out[f] = (ref, bound)
    if kind in ("both", "bf16"):
        out[b] = with_bf16(ref, bound)
    return out


# ------------------------------------------------------------------ ufnd_layernorm
LN_H, LN_M, LN_OUT, LN_EPS = (256, 512, 768, 1024), (1, 3, 4, 5, 130), ("both", "f32", "bf16"), (1e-12, 1e-5)
ROW_KINDS = ("normal", "offset", "spike")      # N(0.5, 3); mean 300, std 1; N(0, 1) with one entry of 1e4


def _ln_cases():
    out, i = [], 0
    for H in LN_H:
        for M in LN_M:      # the other factors rotate: every H meets every stride kind, output form and eps (checked on the CPU)
            out.append((H, M, H + 4 * (i % 2), LN_OUT[i % 3], LN_EPS[(i // 2) % 2], i))
            i += 1
        i += 1
    return out


def ln_rows(rng, M, H, first=0):
    x = np.empty((M, H), dtype=np.float32)
    for r in range(M):
        kind = ROW_KINDS[(first + r) % 3]
        if kind == "normal":
            x[r] = rng.normal(0.5, 3.0, H)
        elif kind == "offset":
            x[r] = rng.normal(300.0, 1.0, H)
        else:
            x[r] = rng.normal(0.0, 1.0, H)
            x[r, int(rng.integers(H))] = 1.0e4
    return x


def _ln_make(case):
    H, M, ldx, _, _, i = case
    rng = _seed(1, H, M, i)
    xs = np.full((M, ldx), np.nan, dtype=np.float32)      # the pad columns of a strided input are never read
    xs[:, :H] = ln_rows(rng, M, H, first=i)
    return dict(x=xs, gamma=_f32(rng.normal(1.0, 0.5, H)), beta=_f32(rng.normal(0.0, 0.5, H)))


def _ln_reference(case, inp):
    H, _, _, kind, eps, _ = case
    return _ref_outs(kind, *ln_ref_bound(inp["x"][:, :H], inp["gamma"].astype(np.float64), inp["beta"].astype(np.float64), eps))


def _ln_restate(case, inp, mutant=None):
    H, _, _, kind, eps, _ = case
    return _outs(kind, ln_f32(inp["x"][:, :H], inp["gamma"], inp["beta"], eps, mutant))


# ------------------------------------------------------------------ ufnd_bert_embed
EMB_VOCAB = 50
EMB_FORMS = (("ln", "f32"), ("ln", "bf16"), ("raw", "f32"), ("raw", "bf16"))


def _emb_cases():
    return [(H, B, L, form, out) for H in LN_H for (B, L) in ((1, 1), (3, 5), (2, 130)) for form, out in EMB_FORMS]


def _emb_make(case):
    H, B, L, _, _ = case
    rng = _seed(2, H, B, L)
    ids = rng.integers(0, EMB_VOCAB, B * L).astype(np.int64)
    edge = [-1, EMB_VOCAB, 2 ** 40, 0, EMB_VOCAB - 1]      # clamp to 0, vocab - 1, vocab - 1
    for k, v in enumerate(edge[:B * L]):
        ids[(k * 7) % (B * L)] = v
    return dict(ids=ids, word=_f32(rng.normal(0, 1, (EMB_VOCAB, H))), pos=_f32(rng.normal(0, 1, (L, H))), type0=_f32(rng.normal(0, 1, H)),
                gamma=_f32(rng.normal(1.0, 0.5, H)), beta=_f32(rng.normal(0.0, 0.5, H)), eps=1e-12)


def _emb_rows(inp, L, dtype, mutant=None):
    ids = inp["ids"]
    rows = np.arange(ids.size)
    if mutant == "no_clamp":
        idc = ids % EMB_VOCAB            # what an unclamped index does at best: wraps
    else:
        idc = np.clip(ids, 0, EMB_VOCAB - 1)
    l = rows // L if mutant == "position_row_div_L" else rows % L
    l = np.clip(l, 0, L - 1)
    w, p, t = inp["word"].astype(dtype), inp["pos"].astype(dtype), inp["type0"].astype(dtype)
    return w[idc], p[l], t


def _emb_reference(case, inp):
    _, _, L, form, out = case
    w, p, t = _emb_rows(inp, L, np.float64)
    s = w + p + t
    # the raw form is two additions, (word + pos) + type: |fl(fl(w + p) + t) - s| <= u |w + p| (1 + u) + u |s|
    ex = U * (np.abs(w + p) * (1 + U) + np.abs(s))
    if form == "raw":
        return _ref_outs(out, s, ex)
    return _ref_outs(out, *ln_ref_bound(s, inp["gamma"].astype(np.float64), inp["beta"].astype(np.float64), inp["eps"], ex))


def _emb_restate(case, inp, mutant=None):
    _, _, L, form, out = case
    w, p, t = _emb_rows(inp, L, np.float32, mutant)
    s = t + (p + w)          # another order than the kernel's
    return _outs(out, s if form == "raw" else ln_f32(s, inp["gamma"], inp["beta"], inp["eps"]))


# ------------------------------------------------------------------ ufnd_vit_assemble
ASM_VARIANTS = ("raw", "ln", "ln_bf16", "ln_stats")


def _asm_cases():
    return [(H, N, P, v) for H in LN_H for (N, P) in ((1, 1), (3, 4), (2, 49)) for v in ASM_VARIANTS]


def _asm_make(case):
    H, N, P, _ = case
    rng = _seed(3, H, N, P)
    return dict(pe=_f32(rng.normal(0, 1, (N * P, H))), cls=_f32(rng.normal(0, 1, H)), pos=_f32(rng.normal(0, 1, (P + 1, H))),
                gamma=_f32(rng.normal(1.0, 0.5, H)), beta=_f32(rng.normal(0.3, 0.5, H)), eps=1e-5)


def _asm_sums(inp, N, P, dtype, mutant=None):
    pe, cls, pos = inp["pe"].astype(dtype), inp["cls"].astype(dtype), inp["pos"].astype(dtype)
    H = cls.size
    x = np.empty((N, P + 1, H), dtype=dtype)
    pidx = (np.arange(P + 1) + 1) % (P + 1) if mutant == "position_shifted_by_one" else np.arange(P + 1)
    if mutant == "class_row_only_for_sample_0":
        flat = np.concatenate([cls[None], pe])[:N * (P + 1)]      # one class row in front of ALL patch rows
        flat = np.concatenate([flat, np.zeros((N * (P + 1) - len(flat), H), dtype)])
        x = flat.reshape(N, P + 1, H) + pos[pidx][None]
        return x.reshape(N * (P + 1), H)
    x[:, 0] = cls + pos[pidx[0]]
    x[:, 1:] = pe.reshape(N, P, H) + pos[pidx[1:]][None]
    return x.reshape(N * (P + 1), H)


def stats_ref_bound(stored):
    """{sum, sum of squares, 0, 0} of the stored fp32 rows; the sums have depth d = 4 NI + 6 (row_stats):
    |d sum| <= d u sum|v|, |d sumsq| <= (d + 1) u sum v^2 (one more for the squares); the two zeros are exact."""
    v = np.asarray(stored, dtype=np.float64)
    d = 4 * (v.shape[-1] // 256) + 6
    ref = np.zeros((v.shape[0], 4))
    bound = np.zeros_like(ref)
    ref[:, 0], ref[:, 1] = v.sum(-1), (v * v).sum(-1)
    bound[:, 0], bound[:, 1] = d * U * np.abs(v).sum(-1), (d + 1) * U * (v * v).sum(-1)
    return ref, bound


def _asm_reference(case, inp):
    H, N, P, variant = case
    s = _asm_sums(inp, N, P, np.float64)
    ex = U * np.abs(s)                                   # one addition
    if variant == "raw":
        return {"of": (s, ex)}
    ref, bound = ln_ref_bound(s, inp["gamma"].astype(np.float64), inp["beta"].astype(np.float64), inp["eps"], ex)
    if variant == "ln_bf16":
        return {"ob": with_bf16(ref, bound)}
    return {"of": (ref, bound)}      # ln_stats: "stats" is compared with stats_ref_bound(of as stored) by the caller


def _asm_restate(case, inp, mutant=None):
    H, N, P, variant = case
    s = _asm_sums(inp, N, P, np.float32, mutant)
    if variant == "raw":
        return {"of": s}
    y = ln_f32(s, inp["gamma"], inp["beta"], inp["eps"])
    if variant == "ln_bf16":
        return {"ob": bf16_round(y)}
    out = {"of": y}
    if variant == "ln_stats":
        v = s if mutant == "stats_before_layernorm" else y
        st = np.zeros((v.shape[0], 4), dtype=np.float32)
        st[:, 0], st[:, 1] = v.sum(-1, dtype=np.float32), (v * v).sum(-1, dtype=np.float32)
        out["stats"] = st
    return out


# ------------------------------------------------------------------ ufnd_vit_patchify (bit equality)
def _pat_cases():
    return [(image, patch, N) for (image, patch) in ((224, 32), (64, 32), (48, 8), (32, 16)) for N in (1, 3)]


def _pat_make(case):
    image, patch, N = case
    return dict(frames=_f32(_seed(4, image, patch, N).normal(0, 1, (N, 3, image, image))))


def _pat_reference(case, inp):
    image, P, N = case
    G = image // P
    x = inp["frames"].reshape(N, 3, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(N * G * G, 3 * P * P)      # (c, ky, kx) inside a patch
    ref = bf16_round(x).astype(np.float64)
    return {"patches": (ref, np.zeros_like(ref))}


def _pat_restate(case, inp, mutant=None):
    image, P, N = case
    G = image // P
    out = np.empty((N * G * G, 3 * P * P), dtype=np.float32)
    ky, kx = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    if mutant == "ky_kx_swapped":
        ky, kx = kx, ky
    for n in range(N):
        for py in range(G):
            for px in range(G):
                for c in range(3):
                    out[(n * G + py) * G + px, c * P * P:(c + 1) * P * P] = inp["frames"][n, c, py * P + ky, px * P + kx].reshape(-1)
    return {"patches": bf16_round(out)}


# ------------------------------------------------------------------ L2 normalisation shared by the pooled ops
def l2_ref_bound(v, dv):
    """out = v / (|v| + 1e-9) for rows v (float64) that carry the elementwise error dv.  The 256-thread norm has depth
    d = ceil(D / 256) + 8; nrm = sqrt(sum v^2) + 1e-9: relative error of the computed norm
      rho = |dv|_2 / nrm + ((d + 1) / 2 + 2) u         the inputs' error; (d + 1) u on the sum of squares halves under the root,
                                                        then the root and the addition
      |d out_k| <= dv_k / nrm + |out_k| (rho + u)       the division"""
    D = v.shape[-1]
    d = -(-D // 256) + 8
    nrm = np.sqrt((v * v).sum(-1, keepdims=True)) + 1e-9
    out = v / nrm
    rho = np.sqrt((dv * dv).sum(-1, keepdims=True)) / nrm + ((d + 1) / 2 + 2) * U
    return out, dv / nrm + np.abs(out) * (rho + U)


def l2_f32(v):
    v = _f32(v)
    return v / (np.sqrt((v * v).sum(-1, keepdims=True, dtype=np.float32), dtype=np.float32) + np.float32(1e-9))


# ------------------------------------------------------------------ ufnd_masked_meanpool_l2
POOL_MASKS = ("prefix", "every_third", "last_only", "none_live")


def _pool_cases():
    return [(H, L) for H in (256, 1024) for L in (1, 31, 32, 33, 77)]


def pool_mask(kind, L, rng):
    m = np.zeros(L, dtype=np.int32)
    if kind == "prefix":
        m[:max(1, int(rng.integers(1, L + 1)))] = 1
    elif kind == "every_third":
        m[::3] = 1
    elif kind == "last_only":
        m[L - 1] = 1
    return m


def _pool_make(case):
    H, L = case
    rng = _seed(5, H, L)
    kinds = list(POOL_MASKS) + ["prefix", "every_third"]      # the last two samples are of size 1e-9 (module docstring)
    B = len(kinds)
    mask = np.stack([pool_mask(k, L, rng) for k in kinds])
    hidden = _f32(rng.normal(0.2, 1.0, (B, L, H)))
    hidden[4:] *= np.float32(2e-10)
    hidden[mask == 0] = np.nan                                # masked positions must never be added
    return dict(hidden=hidden, mask=mask)


def _pool_reference(case, inp):
    """Token sums: group g adds tokens g, g + 4, ... in order (ceil(L / 4) terms), then two levels over the groups:
    d = ceil(L / 4) + 2, one more u for the division by the count; then l2_ref_bound.  No live token: exact zeros."""
    H, L = case
    h, m = inp["hidden"].astype(np.float64), inp["mask"]
    hz = np.where(m[..., None] != 0, h, 0.0)
    n = np.maximum(m.sum(-1, keepdims=True).astype(np.float64), 1e-6)
    pooled = hz.sum(1) / n
    dp = (-(-L // 4) + 3) * U * np.abs(hz).sum(1) / n
    return {"out": l2_ref_bound(pooled, dp)}


def _pool_restate(case, inp, mutant=None):
    H, L = case
    h, m = inp["hidden"], inp["mask"].copy()
    if mutant == "last_live_token_dropped":
        for b in range(m.shape[0]):
            live = np.flatnonzero(m[b])
            if live.size:
                m[b, live[-1]] = 0
    hz = np.where(m[..., None] != 0, h, np.float32(0))
    n = np.maximum(inp["mask"].sum(-1, keepdims=True).astype(np.float32), np.float32(1e-6))
    if mutant == "divide_by_L":
        n = np.full_like(n, L)
    return {"out": l2_f32(hz.sum(1, dtype=np.float32) / n)}


# ------------------------------------------------------------------ ufnd_l2norm_frames
def _frm_cases():
    return [(1, 1, 512), (3, 2, 512), (2, 8, 1024), (2, 3, 300), (2, 2, 1)]


def _frm_make(case):
    B, F, D = case
    rng = _seed(6, B, F, D)
    e = rng.normal(0, 1, (B, F, D))
    e /= np.sqrt((e * e).sum(-1, keepdims=True))
    e *= 10.0 ** rng.uniform(-3, 3, (B, F, 1))      # norms over six decades: "mean, then normalise" is another vector
    if F > 1:
        e[B - 1, 0] *= 1e3 / np.sqrt((e[B - 1, 0] ** 2).sum())
        e[B - 1, F - 1] *= 1e-3 / np.sqrt((e[B - 1, F - 1] ** 2).sum())
    if B > 1 and F > 1:
        e[0, F - 1] = 0.0                            # one all-zero frame: 0 / (0 + 1e-9) = 0
    return dict(e=_f32(e))


def _frm_reference(case, inp):
    """Per frame l2_ref_bound (exact inputs); the mean adds the F unit vectors in order (depth F) and divides: with
    a_k = sum_f |unit_fk| and b_k = sum_f bound_fk, dmean_k = (b_k + (F + 1) u a_k) / F; then l2_ref_bound again.  F = 1: the frame."""
    B, F, D = case
    e = inp["e"].astype(np.float64)
    unit, bu = l2_ref_bound(e, np.zeros_like(e))
    if F == 1:
        return {"out": (unit[:, 0], bu[:, 0])}
    mean = unit.mean(1)
    dmean = (bu.sum(1) + (F + 1) * U * np.abs(unit).sum(1)) / F
    return {"out": l2_ref_bound(mean, dmean)}


def _frm_restate(case, inp, mutant=None):
    B, F, D = case
    e = inp["e"]
    unit = e if mutant == "no_per_frame_normalisation" else l2_f32(e)
    if F == 1:
        return {"out": unit[:, 0]}
    mean = unit.sum(1, dtype=np.float32) / np.float32(F)
    return {"out": mean if mutant == "no_final_normalisation" else l2_f32(mean)}


# ------------------------------------------------------------------ ufnd_field_mean_l2
def _fld_cases():
    return [(4, 12, 768), (3, 1, 300), (2, 5, 1024)]


def _fld_make(case):
    N, Mx, D = case
    rng = _seed(7, N, Mx, D)
    valid = np.zeros((N, Mx), dtype=np.int32)
    valid[0, :] = 1                                  # all parts valid
    if N > 2:
        valid[2, Mx - 1] = 1                         # one valid part (the last)
    if N > 3:
        valid[3, ::2] = 1
    # record 1 has no valid part
    parts = _f32(rng.normal(0.1, 1.0, (N, Mx, D)))
    parts[0] *= np.float32(3e-10)                    # |mean| near 1e-9 (module docstring); with Mx = 1 every divisor is 1
    if N > 3:
        parts[3] *= np.float32(3e-10)
    parts[valid == 0] = np.nan
    return dict(parts=parts, valid=valid)


def _fld_reference(case, inp):
    """Valid parts are added in order (depth cnt) and divided by cnt: dmean = (cnt + 1) u sum|parts| / cnt; then l2_ref_bound.
    A record without a valid part is exact zeros."""
    N, Mx, D = case
    p, v = inp["parts"].astype(np.float64), inp["valid"]
    pz = np.where(v[..., None] != 0, p, 0.0)
    cnt = v.sum(-1, keepdims=True).astype(np.float64)
    c1 = np.maximum(cnt, 1.0)
    return {"out": l2_ref_bound(pz.sum(1) / c1, (cnt + 1) * U * np.abs(pz).sum(1) / c1)}


def _fld_restate(case, inp, mutant=None):
    N, Mx, D = case
    p, v = inp["parts"], inp["valid"]
    pz = np.where(v[..., None] != 0, p, np.float32(0))
    cnt = np.maximum(v.sum(-1, keepdims=True), 1).astype(np.float32)
    if mutant == "divide_by_Mx":
        cnt = np.full_like(cnt, Mx)
    return {"out": l2_f32(pz.sum(1, dtype=np.float32) / cnt)}


# ------------------------------------------------------------------ ufnd_cast_bf16 (bit equality)
def _cast_cases():
    return [1, 3, 4, 5, 1023, CAST_GRID_CAP + 3]      # the last: one sweep past the grid cap and a scalar tail


def cast_specials() -> np.ndarray:
    """+-0, subnormals, +-inf, NaN, and exact ties between two bf16 neighbours (to even: down at ...0, up at ...1)."""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345,
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7F8000, 0x7F7F7FFF, 0x007F8000, 0x3FFF8000]
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _cast_make(n):
    rng = _seed(8, n % 100003)
    x = _f32(rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 6, n))
    sp = cast_specials()
    if n >= 1023:
        x[3:3 + sp.size] = sp
        x[n - sp.size:] = sp[::-1]                   # the scalar tail and the last vector hold them too
    else:
        x[:] = np.resize(np.roll(sp, n), n)
    return dict(x=x)


def _cast_reference(n, inp):
    ref = bf16_round(inp["x"]).astype(np.float64)
    return {"out": (ref, np.zeros_like(ref))}


def _cast_restate(n, inp, mutant=None):
    x = inp["x"]
    if mutant == "truncate":
        return {"out": bf16_f32((x.view(np.uint32) >> 16).astype(np.uint16))}
    if mutant == "ties_away_from_zero":
        b = x.view(np.uint32)
        nan = (b & 0x7FFFFFFF) > 0x7F800000
        return {"out": bf16_f32(np.where(nan, (b >> 16) | 0x40, (b + 0x8000) >> 16).astype(np.uint16))}
    # round to nearest even spelled with arithmetic on the discarded half instead of the carry trick
    b = x.view(np.uint32).astype(np.uint64)
    hi, lo = b >> 16, b & 0xFFFF
    up = (lo > 0x8000) | ((lo == 0x8000) & ((hi & 1) == 1))
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return {"out": bf16_f32(np.where(nan, hi | 0x40, hi + up).astype(np.uint16))}


# ------------------------------------------------------------------ ufnd_act_bf16
ACT_GELU, ACT_QUICK_GELU = 1, 2


def all_finite_bf16() -> np.ndarray:
    b = np.arange(65536, dtype=np.uint32)
    b = b[(b & 0x7F80) != 0x7F80].astype(np.uint16)
    assert b.size == 65280 and b.size % 8 == 0
    return b


def _act_cases():
    return [(act, n) for act in (ACT_GELU, ACT_QUICK_GELU) for n in (65280, ACT_GRID_CAP + 8)]


def _act_make(case):
    act, n = case
    return dict(x=np.resize(all_finite_bf16(), n))


def _erf64(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def _act_reference(case, inp):
    """2^-8 |ref| + 1e-6: one bf16 ulp of the result, and an absolute term for the approximation before the rounding -- the
    polynomial's stated 1.5e-7 erf error times |x| / 2 where the tail is still non-zero (|x| < 6), and the fp32 evaluation."""
    act, _ = case
    x = bf16_f32(all_finite_bf16()).astype(np.float64)
    with np.errstate(over="ignore"):
        ref = 0.5 * x * (1.0 + _erf64(x / math.sqrt(2.0))) if act == ACT_GELU else x / (1.0 + np.exp(-1.702 * x))
    ref = np.resize(ref, inp["x"].size)
    return {"out": (ref, 2.0 ** -8 * np.abs(ref) + 1e-6)}


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _act_restate(case, inp, mutant=None):
    """gelu_fast_f / quick_gelu_fast_f in fp32 (fused multiply-adds rounded once, through float64)."""
    act, n = case
    x = bf16_f32(all_finite_bf16())
    f = np.float32
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == ACT_GELU:
            z = np.abs(x) * f(1.0 if mutant == "erf_without_sqrt2" else 0.70710678118654752440)
            t = f(1) / _fma32(np.full_like(z, 0.3275911), z, f(1))
            c = [1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592]
            p = _fma32(t, np.full_like(t, c[0]), f(c[1]))
            for ck in c[2:]:
                p = _fma32(t, p, f(ck))
            poly = t * p
            e = np.exp((-z * z).astype(np.float64)).astype(f)
            erf_abs = _fma32(-poly, e, f(1))
            h = f(0.5) * x
            y = _fma32(h, np.copysign(erf_abs, x), h)
        else:
            k = 1.0 if mutant == "plain_sigmoid" else 1.702
            m = f(k) * x
            y = x * (f(1) / (np.exp((-m).astype(np.float64)).astype(f) + f(1)))
    return {"out": np.resize(bf16_round(y), n)}


# ------------------------------------------------------------------ ufnd_gather_rows (bit equality)
GATHER_B = 7
GATHER_ITEMS = [(8, 5), (8 * 129, 9), (3072, 6), (16, 64), (24, 7), (512, 11), (8 * 200, 8), (40, 100)]      # (row bytes, source rows)
GATHER_IDX = [4, 0, 0, -3, 5, 8, 2]      # a repeat, a negative, 5 and 8: past the smallest sources; clamped per item


def _gat_make(case):
    rng = _seed(9)
    return dict(idx=np.array(GATHER_IDX, dtype=np.int64), src=[rng.integers(0, 256, (rows, nbytes), dtype=np.uint8) for nbytes, rows in GATHER_ITEMS])


def _gat_reference(case, inp):
    out = {}
    for i, s in enumerate(inp["src"]):
        ref = np.take(s, np.clip(inp["idx"], 0, s.shape[0] - 1), axis=0).astype(np.float64)
        out[f"dst{i}"] = (ref, np.zeros_like(ref))
    return out


def _gat_restate(case, inp, mutant=None):
    out = {}
    smallest = min(s.shape[0] for s in inp["src"])
    for i, s in enumerate(inp["src"]):
        rows = smallest if mutant == "clamp_to_smallest_source" else s.shape[0]
        out[f"dst{i}"] = np.stack([s[min(max(int(j), 0), rows - 1)] for j in inp["idx"]])
    return out


# ------------------------------------------------------------------ ufnd_attention_bf16
ATTN_GRID = [(1, 1, 1), (1, 2, 1), (3, 63, 5), (1, 64, 7), (3, 65, 5), (1, 127, 1), (2, 129, 3), (1, 193, 7), (1, 513, 3), (1, 1100, 1)]
ATTN_MASKS = ("none", "prefix", "left", "hole", "single")      # sample 1 of a masked launch with B > 1 is all-masked
KB = 64                                                          # keys per block of the kernel
SELECT_MARGIN = 40.0                                             # nats


def attn_mask_row(kind, L):
    m = np.ones(L, dtype=np.int32)
    if kind == "prefix":
        m[max(1, L // 3):] = 0
    elif kind == "left":                    # the first key block (and more) is masked when L > 96
        m[:min(L - 1, max(1, 2 * L // 3))] = 0
    elif kind == "hole":                    # a whole key block when there is one with live keys on both sides
        if L > 2 * KB:
            m[KB:2 * KB] = 0
        else:
            m[L // 3:max(L // 3 + 1, 2 * L // 3)] = 0
            m[L - 1] = 1
    elif kind == "single":
        m[:] = 0
        m[L - 1] = 1
    elif kind == "all_masked":
        m[:] = 0
    return m


def attn_mask(kind, B, L) -> Optional[np.ndarray]:
    if kind == "none":
        return None
    order = [kind, "all_masked"] + [k for k in ATTN_MASKS[1:] if k != kind]
    return np.stack([attn_mask_row(order[b % len(order)], L) for b in range(B)])


def _attn_cases():
    return [(B, L, heads, kind) for (B, L, heads) in ATTN_GRID for kind in ATTN_MASKS]


def attn_grid_size(B, L, heads) -> int:
    return heads * B if L <= ATTN_SHORT_L else -(-L // 128) * heads * B


def _split(qkv_bits, B, L, heads):
    """(B L, 3 H) bf16 bits -> q, k, v float64 of shape (B, heads, L, 64)"""
    x = bf16_f32(qkv_bits).astype(np.float64).reshape(B, L, 3, heads, 64)
    return tuple(x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))


def attn_ref_bound(qkv_bits, mask, B, L, heads):
    """float64 softmax attention of the bf16 operands (a masked key has probability 0; a sample without a live key averages
    all L keys: HF's finfo.min arithmetic) and the elementwise bound.  With A_id = sum_j P_ij |V_jd|, T_ij = sum_d |q_id k_jd|:
      delta_i = 8 u max_j T_ij + 4 u max_j |s_ij| + 2^-23      relative error of an unnormalised p_ij: the 64-term fp32 dot product
                                                               times 1/8, the scaling and the subtraction of the maximum (at
                                                               most twice the largest score), v_exp_f32 at 1 ulp
      e1 = (2 delta_i + (L + 2 nblk + 24) u) A + BF A          p's error in the numerator and in l; the P V sum (depth <= L), one
                                                               rescale per key block, l's own sum (16 per lane and block, the
                                                               blocks, two shuffles), 1 / l and the product; P rounded to bf16
                                                               in the numerator only (l adds the unrounded p)
      bound = e1 + BF (|ref| + e1)                             the output's rounding to bf16"""
    q, k, v = _split(qkv_bits, B, L, heads)
    s = np.einsum("bhid,bhjd->bhij", q, k) * 0.125
    T = np.einsum("bhid,bhjd->bhij", np.abs(q), np.abs(k))
    live = np.ones((B, L), dtype=bool) if mask is None else mask != 0
    dead = ~live.any(-1)                                    # no live key: every score IS the mask constant, the softmax is uniform
    s = np.where(dead[:, None, None, None], 0.0, s)
    live = np.where(live.any(-1, keepdims=True), live, True)[:, None, None, :]
    sm = np.where(live, s, -np.inf)
    p = np.exp(sm - sm.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhij,bhjd->bhid", p, v)
    A = np.einsum("bhij,bhjd->bhid", p, np.abs(v))
    delta = 8 * U * np.where(live, T, 0).max(-1, keepdims=True) + 4 * U * np.where(live, np.abs(s), 0).max(-1, keepdims=True) + HW_ULP
    nblk = -(-L // KB)
    e1 = (2 * delta + (L + 2 * nblk + 24) * U) * A + BF * A
    bound = e1 + BF * (np.abs(ref) + e1)
    merge = lambda t: t.transpose(0, 2, 1, 3).reshape(B * L, heads * 64)
    return merge(ref), merge(bound)


def attn_f32(qkv_bits, mask, B, L, heads, mutant=None):
    """fp32 attention with the kernel's roundings (P to bf16 in the numerator, the output to bf16), no key blocks."""
    q, k, v = (t.astype(np.float32) for t in _split(qkv_bits, B, L, heads))
    s = np.einsum("bhid,bhjd->bhij", q, k) * np.float32(0.125)
    live = np.ones((B, L), dtype=bool) if mask is None else mask != 0
    if mutant == "mask_shifted_by_one" and mask is not None:
        live = np.roll(live, 1, axis=-1)
    dead = ~live.any(-1)
    s = np.where(dead[:, None, None, None], np.float32(0), s)
    live = np.where(live.any(-1, keepdims=True), live, True)
    if mutant == "last_key_of_a_block_dropped":
        cut = live & (np.arange(L) % KB != KB - 1)[None]
        live = np.where(cut.any(-1, keepdims=True), cut, live)      # (never the only live key: the softmax stays defined)
    live = live[:, None, None, :]
    sm = np.where(live, s, -np.inf).astype(np.float32)
    p = np.exp(sm - sm.max(-1, keepdims=True), dtype=np.float32)
    l = p.sum(-1, keepdims=True, dtype=np.float32)
    o = np.einsum("bhij,bhjd->bhid", bf16_round(p), v).astype(np.float32) / l
    if mutant == "all_masked_row_is_zeros":
        o[dead] = 0
    return bf16_round(o.transpose(0, 2, 1, 3).reshape(B * L, heads * 64))


def _pack_qkv(q, k, v):
    """(B, heads, L, 64) x 3 float -> (B L, 3 H) bf16 bits"""
    B, heads, L, _ = q.shape
    x = np.stack([q, k, v], 0).transpose(1, 3, 0, 2, 4).reshape(B * L, 3 * heads * 64)
    return bf16_bits(x)


# selection probe: query i is the key at pi(i), a permutation of the live keys (reused cyclically for the queries beyond them)
def select_inputs(case):
    B, L, heads, kind = case
    rng = _seed(10, B, L, heads, ATTN_MASKS.index(kind))
    mask = attn_mask(kind, B, L)
    k = rng.choice([-4.0, 4.0], (B, heads, L, 64))
    mag = rng.choice([0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 3.5, 5.0, 6.0, 7.0, 8.0], (B, heads, L, 64))      # bf16-exact, 0.5 <= |v| <= 8
    v = mag * rng.choice([-1.0, 1.0], mag.shape)
    pi = np.zeros((B, heads, L), dtype=np.int64)
    for b in range(B):
        live = np.arange(L) if mask is None or not mask[b].any() else np.flatnonzero(mask[b])
        for h in range(heads):
            pi[b, h] = np.resize(rng.permutation(live), L)
    q = np.take_along_axis(k, pi[..., None], axis=2)
    return dict(qkv=_pack_qkv(q, k, v), mask=mask, pi=pi)


def select_margin(case, inp) -> float:
    """The least (selected score - any other live score of the row), in nats, over the samples that have a live key."""
    B, L, heads, _ = case
    q, k, _ = _split(inp["qkv"], B, L, heads)
    s = np.einsum("bhid,bhjd->bhij", q, k) * 0.125
    mask = inp["mask"]
    worst = math.inf
    for b in range(B):
        if mask is not None and not mask[b].any():
            continue
        live = np.ones(L, dtype=bool) if mask is None else mask[b] != 0
        for h in range(heads):
            sel = np.take_along_axis(s[b, h], inp["pi"][b, h][:, None], axis=1)
            other = np.where(live[None, :], s[b, h], -np.inf)
            np.put_along_axis(other, inp["pi"][b, h][:, None], -np.inf, axis=1)
            if L > 1 and np.isfinite(other).any():
                worst = min(worst, float((sel[:, 0] - other.max(-1)).min()))
    return worst


def _select_reference(case, inp):
    """ctx[i] == V[pi(i)] bit for bit: every other probability is below exp(-40) = 5e-18, far under half an fp32 ulp of l = 1 and
    of any |v| >= 0.5, and v is bf16-exact.  A sample without a live key has nothing to select: there the general bound holds."""
    B, L, heads, _ = case
    _, _, v = _split(inp["qkv"], B, L, heads)
    sel = np.take_along_axis(v, inp["pi"][..., None], axis=2).transpose(0, 2, 1, 3).reshape(B * L, heads * 64)
    exact = np.ones(B, dtype=bool) if inp["mask"] is None else inp["mask"].any(-1)
    if exact.all():
        return {"ctx": (sel, np.zeros_like(sel))}
    ref, bound = attn_ref_bound(inp["qkv"], inp["mask"], B, L, heads)
    rows = np.repeat(exact, L)[:, None]
    return {"ctx": (np.where(rows, sel, ref), np.where(rows, 0.0, bound))}


# census probe: Q = 0 and V[j][d] = (j % 64 == d), so ctx[i][d] = (live keys congruent to d) / (live keys)
def census_inputs(case):
    B, L, heads, kind = case
    z = np.zeros((B, heads, L, 64))
    v = np.broadcast_to((np.arange(L)[:, None] % 64 == np.arange(64)[None, :]).astype(np.float64), (B, heads, L, 64))
    k = _seed(11, B, L, heads).choice([-2.0, 0.5, 3.0], (B, heads, L, 64))      # any keys: Q = 0 makes every score 0
    return dict(qkv=_pack_qkv(z, k, v), mask=attn_mask(kind, B, L))


def _census_reference(case, inp):
    """Every live key has p = exp2(0) = 1 exactly, l = n, the numerators are whole counts: the only roundings are 1 / l, the product
    and the bf16 output -- one bf16 ulp of the value is accepted (0 must be 0).  A lost or doubled key moves a channel by at least
    1 / 18 of its value (counts <= 18 at L <= 1100) against 2^-8 of it."""
    B, L, heads, _ = case
    mask = inp["mask"]
    live = np.ones((B, L), dtype=bool) if mask is None else mask != 0
    live = np.where(live.any(-1, keepdims=True), live, True)
    onehot = (np.arange(L)[:, None] % 64 == np.arange(64)[None, :])
    cnt = (live[:, :, None] & onehot[None]).sum(1).astype(np.float64)      # (B, 64)
    val = cnt / live.sum(-1, keepdims=True)
    ref = np.broadcast_to(val[:, None, None, :], (B, L, heads, 64)).reshape(B * L, heads * 64)
    return {"ctx": (ref.copy(), bf16_ulp(ref))}


def general_inputs(case):
    B, L, heads, kind = case
    rng = _seed(12, B, L, heads)
    return dict(qkv=bf16_bits(_f32(rng.normal(0, 1, (B * L, 3 * heads * 64)) * 1.5)), mask=attn_mask(kind, B, L))


def _general_reference(case, inp):
    B, L, heads, _ = case
    return {"ctx": attn_ref_bound(inp["qkv"], inp["mask"], B, L, heads)}


def _attn_restate(case, inp, mutant=None):
    B, L, heads, _ = case
    return {"ctx": attn_f32(inp["qkv"], inp["mask"], B, L, heads, mutant)}


ATTN_MUTANTS = ("last_key_of_a_block_dropped", "mask_shifted_by_one", "all_masked_row_is_zeros")

OPS: Dict[str, Op] = {
    "layernorm": Op(_ln_cases(), _ln_make, _ln_reference, _ln_restate, ("one_pass_variance", "divide_by_h_minus_1", "beta_before_gamma")),
    "bert_embed": Op(_emb_cases(), _emb_make, _emb_reference, _emb_restate, ("position_row_div_L", "no_clamp")),
    "vit_assemble": Op(_asm_cases(), _asm_make, _asm_reference, _asm_restate,
                       ("position_shifted_by_one", "class_row_only_for_sample_0", "stats_before_layernorm")),
    "vit_patchify": Op(_pat_cases(), _pat_make, _pat_reference, _pat_restate, ("ky_kx_swapped",)),
    "masked_meanpool_l2": Op(_pool_cases(), _pool_make, _pool_reference, _pool_restate, ("divide_by_L", "last_live_token_dropped")),
    "l2norm_frames": Op(_frm_cases(), _frm_make, _frm_reference, _frm_restate, ("no_per_frame_normalisation", "no_final_normalisation")),
    "field_mean_l2": Op(_fld_cases(), _fld_make, _fld_reference, _fld_restate, ("divide_by_Mx",)),
    "cast_bf16": Op(_cast_cases(), _cast_make, _cast_reference, _cast_restate, ("truncate", "ties_away_from_zero")),
    "act_bf16": Op(_act_cases(), _act_make, _act_reference, _act_restate, ("erf_without_sqrt2", "plain_sigmoid")),
    "gather_rows": Op([("one_launch",)], _gat_make, _gat_reference, _gat_restate, ("clamp_to_smallest_source",)),
    "attention_select": Op(_attn_cases(), select_inputs, _select_reference, _attn_restate, ATTN_MUTANTS),
    "attention_census": Op(_attn_cases(), census_inputs, _census_reference, _attn_restate, ATTN_MUTANTS),
    "attention_general": Op(_attn_cases(), general_inputs, _general_reference, _attn_restate, ATTN_MUTANTS),
}


def case_id(case) -> str:
    return "-".join(str(c) for c in case) if isinstance(case, tuple) else str(case)


def check(op: str, case, inp, got: Dict[str, np.ndarray], refs=None) -> Dict[str, float]:
    """error / bound of every output of a case (the vit_assemble statistics are judged against the stored fp32 rows); refs = a
    reference(case, inp) computed earlier."""
    refs = dict(OPS[op].reference(case, inp) if refs is None else refs)
    if "stats" in got:
        refs["stats"] = stats_ref_bound(got["of"])
    assert set(refs) == set(got), (op, case, sorted(refs), sorted(got))
    return {k: worst_ratio(got[k], *refs[k]) for k in refs}
