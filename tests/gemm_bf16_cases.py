"""Case table, float64 references and per-element bounds of the one-tile bf16 GEMM (csrc/gemm_bf16_kernel.hpp: every nn.Linear of both
encoders -- plain, LayerNorm-folded, residual through a LayerNorm -- and, as the BWD instantiation, the backward input gradient),
shared by tests/test_gemm_bf16_cases.py (CPU: the table reaches what it claims, read from the library's own host-side checks and
choice; the bounds accept a float32 restatement of the kernel in two summation orders and reject thirteen wrong kernels) and
tests/test_gpu_gemm_bf16.py (GPU: every case through the C ABI).  NumPy only.  The persistent form of the same arithmetic
(csrc/gemm_bf16_pp.hpp, tile id 64, K = 768) has its table in tests/gemm_pp_cases.py, built on the functions and bounds of this file.

A case is ONE launch of ufnd_gemm_bf16 ("gemm"), ufnd_gemm_bf16_ex ("ex"), ufnd_gemm_bf16_ln ("ln") or ufnd_gemm_bf16_dgrad ("dgrad").
Shapes are the smallest that reach an edge: K = 64 .. 320 (nk = K / 64 = 1 .. 5 straddles every ring depth, 2 .. 4), two to four
column tiles, a handful of row tiles; only the dgrad cases that the automatic choice must send to tiles 22 and 15 need a few thousand
rows (K = 64 there).

TWO DATA FAMILIES
  exact    bf16 operands are multiples of 1/4 in [-2, 2]: a product is a multiple of 1/16 of at most 4, so every partial sum of up
           to 320 of them is a multiple of 1/16 below 1,280 -- exact in fp32 IN ANY ORDER (16 x 1,280 < 2^24).  Bias and residual are
           multiples of 1/16 below 2,048, so each epilogue add is exact too (the sum stays a multiple of 1/16 below 2^14).  With no
           activation and no LayerNorm the fp32 output must EQUAL the float64 result and the bf16 output its round-to-nearest-even:
           the bound is 0.  Every indexing concern (strides, the XCD remap, ragged rows, the ends of the K loop, in-place) runs on
           this family: a wrong index yields another integer.  Rows of A, rows of W, bias entries and residual rows are pairwise
           different (asserted in make()).  Where a LayerNorm or an activation follows, the operands are still these integers (the
           accumulation term of the bound is 0) and the remaining terms are the rounded family's.
  rounded  A ~ N(0, 1) (+ a per-row offset in the LayerNorm forms), W ~ N(0, 1) / sqrt(K), real bias / residual / gamma / beta.

BOUNDS (rounded arithmetic; U = 2^-24 is one correctly rounded fp32 operation, relative; every term first order plus the products of
the terms where two errors multiply).  None was chosen from a GPU result.
  accumulation   acc = sum_k a_k w_k.  A bf16 x bf16 product is exact in fp32 (16 significand bits); the K - 1 additions happen inside
                 the MFMA (32 k per instruction) and between MFMAs, in an order the ISA reference does not fix and with an adder it does
                 not promise to be round-to-nearest, so each addition is charged one ULP (2^-23) of the running magnitude:
                 |acc - exact| <= K 2^-23 sum_k |a_k w_k|.                                                            [ACC_ULP]
  folded LN      (ufnd_gemm_bf16_ln's header: rstd (A W'^T - mean colsum) + bias').  The reference takes the SAME fp32 partials and
                 forms mean and rstd in float64; the kernel adds the P = a_parts partials in fp32 (<= P U sum |partial| each for the sum
                 and the sum of squares), mean = fl(sm inv_h), var = fl(fma(-mean, mean, fl(sq inv_h))) (>= 0), rstd = v_rsq_f32(var + eps):
                 1 ulp, 2^-23.  d_mean, d_var and d_rstd = rstd (d_var / (2 (var + eps)) + 2^-23 + U) follow per row (row_stats()).
                 t = fma(-mean, colsum, acc): e_t = e_acc + d_mean |colsum| + U |t|;  v = fl(rstd t): e = d_rstd |t| + rstd e_t + U |v|.
  bias           v = fl(v + bias): + U |v| (0 in the exact family while nothing inexact has happened).
  activation     y = act(v) against the exact erf-GELU / x sigmoid(1.702 x) in float64: |act'| <= 1.13 times the incoming error, plus
                 the approximation: ACT_ABS[act] (the float32 restatement of gelu_fast / quick_gelu_fast against float64 over
                 |x| <= ACT_RANGE, measured on the CPU by measure_act_errors(): Abramowitz-Stegun 7.1.26's 1.5e-7 |x| / 2 and the fp32
                 evaluation) plus what the hardware's v_exp_f32 and v_rcp_f32 (1 ulp each) may add beyond the restatement's correctly
                 rounded ones: GELU: e = exp(-z^2) through exp2(x log2 e): 2^-23 (e + z^2 e) <= 1.4 x 2^-23 on erf, i.e. 0.7 x 2^-23 |x|
                 on the result; t = rcp(..): |d poly / dt| <= sum k |c_k| = 16.2, t e <= 1: 8.1 x 2^-23 |x|: together 9 x 2^-23 |x|.
                 quick-GELU: y = x s, s = rcp(1 + exp(-m)): ds / s <= (1 - s)(1 + |m|) 2^-23 + 2^-23 + U, and (1 - s) |m| s <= 0.28 s:
                 4 x 2^-23 |x|.                                                                                      [ACT_HW]
  residual       fp32 or bf16 values are exact inputs.  Through a LayerNorm: r' = fma(fl(fl(r - mean) rstd), gamma, beta):
                 e1 = d_mean + U |r - mean|; e2 = |r - mean| d_rstd + rstd e1 + U |.|; e_r = |gamma| e2 + U |r'|.  v = fl(v + r'): + U |v|.
  out_bf16       half a bf16 ulp on top of the fp32 bound e, taken exactly: rounding is monotone, so the stored value must lie in
                 [RNE(ref - e), RNE(ref + e)] (this is never wider than e + half an ulp, and it is the round-to-nearest-even of the
                 reference itself where e = 0).  The figure reported is the fraction of e needed to explain the stored value: the
                 distance from the reference to the nearest real number that rounds to it, over e (bf16_ratio()); 0 = it is RNE(ref).
  out_stats      {sum, sum of squares} of each aligned 32 columns of the fp32 row, against the float64 sums of the float64 output:
                 sum: sum e_v + 32 U sum |v|;  squares: sum (2 |v| e_v + e_v^2) + 33 U sum v^2 (32 fma + 31 additions, any order).
  guard          max over the live rows of fl(|mean| rstd): per row (d_mean rstd + |mean| d_rstd + U |mean| rstd), the bound of the
                 maximum is the largest row bound; slots no workgroup owns keep their zero; a NaN statistic reports +inf.
  dgrad          out = fl(acc g), g = act'(aux) in fp32: e = |g| e_acc + |acc| E_g + e_acc E_g + U |out|.  gelu_grad_f = cdf + x pdf with
                 libm's erff (OpenCL's accuracy ceiling, 16 ulp, is what is promised: 16 x 2^-23 on erf, half of it on cdf) and __expf
                 (x pdf (1 + x^2 / 2) 2^-23 x 2 <= 1.3 x 2^-23): 12 x 2^-23, plus GRAD_ABS (the restatement's own roundings, measured).
                 quick_gelu_grad_f = s (1 + 1.702 x (1 - s)): qgrad_bound(x), evaluated per element.  + fp32 residual: + U |out|.

POISON AND SENTINELS.  Every operand is POST rows longer than the launch may read and its pad columns (between the tight width and the
stride) and extra rows hold NaN -- A, W, residual, residual_bf16, aux, bias / colsum / gamma / beta past N, statistics rows past M: a
K loop one step long or an epilogue one column off puts a NaN into a stored element or the guard.  Every output has PRE rows in front
and POST behind and pad columns, all holding a sentinel that must survive (check() returns inf otherwise).  Nothing is placed against
the end of an allocation."""
from __future__ import annotations

import math
import zlib
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from tests.frozen_ops_cases import BF, HW_ULP, U, bf16_bits, bf16_f32, bf16_round, bf16_ulp, worst_ratio  # noqa: F401

ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_GELU_BWD, ACT_QUICK_GELU_BWD = 0, 1, 2, 3, 4
ACC_ULP = 2.0 ** -23
ACT_HW = {ACT_GELU: 9 * HW_ULP, ACT_QUICK_GELU: 4 * HW_ULP}
ACT_SLOPE = 1.13                  # sup |GELU'| = 1.129, sup |quick-GELU'| = 1.100
ACT_RANGE = 10.0                  # |argument| of every activation in the table (asserted in reference())
GELU_GRAD_HW = 12 * HW_ULP
MUTANT_FACTOR = 4.0               # a mutant must leave a bound by this factor (or break an exact equality) on its case
PRE, POST = 2, 3                  # sentinel rows in front of / behind every output; NaN rows behind every input
VEC_PAD = 8                       # NaN elements behind bias / colsum / gamma / beta
SENT_F32 = np.float32(12345.678)
SENT_BF16 = np.uint16(0x4E4E)
NAN_BF16 = np.uint16(0x7FC0)
GUARD_SLOTS = 1024
EPS = 1e-5

# the tile table of csrc/gemm_bf16_kernel.hpp's product tiles: id -> (bm, bn, A ring depth, W ring depth, wave-tile columns).  The CPU
# test compares it with ufnd_gemm_bf16_tile_info and the diagnostics plan entry: a tile added to or dropped from the library fails there.
TILES = {2: (256, 128, 3, 3, 64), 8: (256, 192, 2, 2, 96), 15: (256, 256, 2, 2, 128), 16: (128, 128, 3, 3, 64), 17: (128, 192, 3, 3, 96),
         20: (128, 64, 4, 4, 32), 22: (256, 192, 3, 2, 96), 28: (256, 144, 2, 2, 144)}
LN_TILES = tuple(TILES)            # every product tile has the LayerNorm-aware kernel
BWD_TILES = (15, 16, 17, 20, 22)
A_PARTS = (2, 4, 10, 22, 24)
R_PARTS = (2, 12, 24)
# the persistent form (csrc/gemm_bf16_pp.hpp; UFND_GEMM_TILE_PERSISTENT) is not a row of the library's tile table and has no case in
# CASES: its table is tests/gemm_pp_cases.py, which shares everything below.  Its workgroups walk 256 x 128 tiles (A ring 3, W ring 2,
# wave tile 64 columns); the grid is G = min(CUs, tiles) & ~7, PP_CUS where nobody names the device's count.
PP_TILE = 64
PP_DIMS = (256, 128, 3, 2, 64)
PP_CUS = 256


def tile_dims(tile: int):
    """(bm, bn, A ring depth, W ring depth, wave-tile columns) of a product tile or of the persistent form"""
    return PP_DIMS if tile == PP_TILE else TILES[tile]


def has_stats_epilogue(tile: int, N: int) -> bool:
    """stat_parts_for / pp_stat_parts: 32-column groups must not straddle a wave tile (tile 28: 144 columns), N / 32 even and <= 24"""
    return tile_dims(tile)[4] % 32 == 0 and N % tile_dims(tile)[1] == 0 and (N // 32) % 2 == 0 and N // 32 <= 24


class Case(NamedTuple):
    id: str
    entry: str                    # gemm | ex | ln | dgrad
    tile: int                     # forced tile (ex, ln); -1: the automatic choice (gemm, dgrad), `want` names the tile it must reach
    want: int
    M: int
    N: int
    K: int
    family: str                   # exact | rounded
    lda: int
    ldw: int
    ldr: int
    ldo: int
    ldf: int
    ldrb: int
    ldaux: int
    bias: bool
    res: str                      # none | f32 | bf16 | inplace (out_f32 aliases the fp32 residual)
    outs: str                     # bf16 | f32 | both
    act: int
    ln: str                       # none | fold | rln | plain (the ln entry with neither a_stats nor r_stats)
    parts: int                    # a_parts / r_parts
    guard: str                    # no | yes | nan (one live row's statistics are NaN: the guard must report +inf)
    out_stats: bool
    refuse: str                   # "": the launch runs; otherwise the words of the refusal the entry must answer with
    edge: str


def _mk(entry, tile, M, N, K, family, *, want=None, tight=False, bias=True, res="none", outs="both", act=0, ln="none", parts=0,
        guard="no", out_stats=False, refuse="", edge="", tag=""):
    # default strides: all different and all wider than the tight value (a swapped pair of strides changes the addresses)
    s = dict(lda=K, ldw=K, ldr=N, ldo=N, ldf=N, ldrb=N, ldaux=N) if tight else \
        dict(lda=K + 8, ldw=K + 16, ldr=N + 20, ldo=N + 24, ldf=N + 28, ldrb=N + 32, ldaux=N + 40)
    if res == "inplace":
        s["ldr"] = s["ldf"]
    want = tile if want is None else want
    bits = [entry, f"t{want}", f"{M}x{N}x{K}", family[0], ln if ln != "none" else "", f"p{parts}" if parts else "", f"a{act}" if act else "",
            "b" if bias else "nb", f"r{res}" if res != "none" else "", f"o{outs}", "g" + guard if guard != "no" else "",
            "os" if out_stats else "", "tight" if tight else "", "refused" if refuse else "", tag]
    return Case("-".join(b for b in bits if b), entry, tile, want, M, N, K, family, bias=bias, res=res, outs=outs, act=act, ln=ln,
                parts=parts, guard=guard, out_stats=out_stats, refuse=refuse, edge=edge, **s)


REFUSE_STATS = "out_stats unsupported for this shape / tile"


def nk_values(tile: int) -> List[int]:
    """nk below, at and above both ring depths of a tile"""
    _, _, sta, stb, _ = TILES[tile]
    return sorted({d + o for d in (sta, stb) for o in (-1, 0, 1)})


def _cases() -> List[Case]:
    out: List[Case] = []
    for t, (bm, bn, sta, stb, _) in TILES.items():
        n2 = 2 * bn if (2 * bn) % 64 == 0 else 4 * bn      # two column tiles (tile 28: N must be a multiple of 64 and of 144: four)
        # ---- the K loop: prologue, the three drain loops, the STA <= nk wait choice; the LayerNorm-aware kernel's "slot whose step
        # does not exist" path is nk < sta.  Two row tiles (the second holds ONE live row), two column tiles.
        for nk in nk_values(t):
            M, N, K = bm + 1, n2, 64 * nk
            edge = f"nk={nk} against ring depths A {sta} / W {stb}"
            out.append(_mk("ex", t, M, N, K, "exact", res="f32", edge=edge))
            out.append(_mk("ln", t, M, N, K, "exact", ln="fold", parts=A_PARTS[nk % 5], guard="yes", edge=edge))
            out.append(_mk("ln", t, M, N, K, "exact", ln="rln", parts=R_PARTS[nk % 3], res="f32" if nk % 2 else "bf16", edge=edge))
            out.append(_mk("ln", t, M, N, K, "exact", ln="plain", res="bf16", outs="bf16", out_stats=has_stats_epilogue(t, N), edge=edge))
        # ---- ragged rows
        for M in (1, bm - 1):
            out.append(_mk("ex", t, M, n2, 128, "exact", res="f32", edge=f"M={M} against bm={bm}"))
        # ---- the grid: column halves (xcd_cols = 2), the remap's remainder, four row tiles with an odd column-tile count.  N must be
        # a multiple of 64 AND of bn: tile 28 (bn = 144) only has column-tile counts that are multiples of 4, so its odd cases do not exist
        out.append(_mk("ex", t, 3 * bm + 5, n2, 128, "exact", res="f32", edge="m_tiles = 4, an even n_tiles: xcd_cols = 2"))
        if (3 * bn) % 64 == 0:
            out.append(_mk("ex", t, 2 * bm + 37, 3 * bn, 64, "exact", res="f32", edge="9 tiles: remap q = 1, r = 1"))
            out.append(_mk("ex", t, 3 * bm + 5, 3 * bn, 64, "exact", res="f32", edge="m_tiles = 4, n_tiles = 3 (odd): row-major, r = 4"))
        else:
            out.append(_mk("ex", t, 2 * bm + 37, 4 * bn, 64, "exact", res="f32", edge="12 tiles: remap q = 1, r = 4 (no odd count exists)"))
        # ---- residual through a LayerNorm on every LayerNorm-aware tile (FIXCOL and !FIXCOL epilogues; tile 28: N = 4 x 144)
        N = n2
        for res in ("f32", "bf16"):
            for parts in R_PARTS:
                for os_ in (False, True):
                    ok = has_stats_epilogue(t, N) or not os_
                    out.append(_mk("ln", t, bm + 3, N, 128, "rounded", ln="rln", parts=parts, res=res, out_stats=os_,
                                   outs="bf16" if res == "bf16" else "both", refuse="" if ok else REFUSE_STATS,
                                   edge="LayerNorm of the residual" + ("" if ok else "; no statistics epilogue: refused")))
        # ---- both families per form
        out.append(_mk("ex", t, bm + 1, n2, 192, "rounded", res="f32", act=1 + t % 2, edge="rounded data, activation"))
        out.append(_mk("ln", t, bm + 1, N, 192, "rounded", ln="plain", res="bf16", outs="bf16", out_stats=has_stats_epilogue(t, N),
                       edge="the ViT's stream: bf16 residual, statistics out"))
    # ---- the plain epilogue's arms, on the automatic choice (tile 20): exact without an activation, rounded with one
    for bias in (True, False):
        for act in (0, 1, 2):
            for res in ("f32", "none"):
                for outs in ("bf16", "f32", "both"):
                    out.append(_mk("gemm", -1, 130, 128, 128, "rounded" if act else "exact", want=20, bias=bias, act=act, res=res, outs=outs,
                                   edge="epilogue arm"))
    out.append(_mk("gemm", -1, 130, 128, 128, "rounded", want=20, res="f32", edge="rounded data, no activation"))
    out.append(_mk("gemm", -1, 130, 128, 128, "exact", want=20, res="inplace", outs="f32", edge="in place: out_f32 = residual"))
    out.append(_mk("ex", 17, 130, 192, 128, "exact", res="inplace", outs="both", edge="in place on a !FIXCOL tile"))
    out.append(_mk("gemm", -1, 130, 128, 128, "exact", want=20, res="f32", tight=True, edge="tight strides"))
    out.append(_mk("gemm", -1, 1, 64, 64, "exact", want=20, res="f32", edge="the smallest launch: nk = 1 < depth 4"))
    # ---- the folded LayerNorm: activation x partial count x guard, and the NaN statistic
    for act in (0, 1, 2):
        for parts in A_PARTS:
            for guard in ("no", "yes"):
                out.append(_mk("ln", 20, 130, 128, 128, "rounded", ln="fold", act=act, parts=parts, guard=guard, edge="folded LayerNorm"))
    for t in (16, 17, 28):
        out.append(_mk("ln", t, TILES[t][0] + 3, 576 if t == 28 else 2 * TILES[t][1], 192, "rounded", ln="fold", act=1, parts=10, guard="yes",
                       edge="folded LayerNorm, rounded data, nk = depth"))
    out.append(_mk("ln", 20, 130, 128, 128, "rounded", ln="fold", parts=4, guard="nan", edge="a NaN statistic must report +inf"))
    out.append(_mk("ln", 20, 130, 128, 64, "rounded", ln="fold", parts=24, guard="yes", act=2, tight=True, edge="nk = 1 < 4: fillers; tight strides"))
    out.append(_mk("ln", 20, 130, 128, 128, "exact", ln="plain", res="f32", edge="the ln entry, nothing folded, fp32 residual"))
    # ---- dgrad: every BWD tile through the automatic choice with ragged M (K = 64 at the large shapes), then the epilogue's arms
    big = {20: (130, 128), 16: (130, 2048), 17: (130, 3072), 22: (9 * 256 + 7, 3072), 15: (23 * 256 + 7, 2048)}
    for t, (M, N) in big.items():
        out.append(_mk("dgrad", -1, M, N, 64, "exact", want=t, bias=False, res="f32", edge=f"automatic choice -> tile {t}, ragged M"))
        out.append(_mk("dgrad", -1, M, N, 64, "exact", want=t, bias=False, outs="bf16", edge=f"automatic choice -> tile {t}, no residual"))
    for act, res in ((0, "none"), (0, "f32"), (ACT_GELU_BWD, "none"), (ACT_QUICK_GELU_BWD, "none")):
        for outs in ("bf16", "f32", "both"):
            out.append(_mk("dgrad", -1, 130, 128, 192, "rounded", want=20, bias=False, act=act, res=res, outs=outs, edge="dgrad epilogue arm"))
    for t in (16, 17):
        for act in (ACT_GELU_BWD, ACT_QUICK_GELU_BWD):
            out.append(_mk("dgrad", -1, 130, big[t][1], 64, "rounded", want=t, bias=False, act=act, outs="bf16", edge="activation backward, strided aux"))
    out.append(_mk("dgrad", -1, 130, 128, 128, "exact", want=20, bias=False, res="f32", tight=True, edge="tight strides"))
    return out


CASES: List[Case] = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids collide"


def tile_of(c: Case) -> int:
    return c.want


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatements of the device's activation functions (fused multiply-adds rounded once, through float64)
f32 = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _exp32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(x, np.float64)).astype(f32)


def _erf64(x):
    return np.vectorize(math.erf, otypes=[np.float64])(np.asarray(x, np.float64))


def gelu_fast_f32(x):
    x = np.asarray(x, f32)
    z = np.abs(x) * f32(0.70710678118654752440)
    t = (1.0 / _fma(f32(0.3275911), z, f32(1)).astype(np.float64)).astype(f32)
    p = _fma(t, f32(1.061405429), f32(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = _fma(t, p, f32(c))
    poly = t * p
    erf_abs = _fma(-poly, _exp32(-z * z), f32(1))
    h = f32(0.5) * x
    return _fma(h, np.copysign(erf_abs, x), h)


def quick_gelu_fast_f32(x, k=1.702):
    x = np.asarray(x, f32)
    d = _exp32(-(f32(k) * x)) + f32(1)
    return x * (1.0 / d.astype(np.float64)).astype(f32)


def gelu_grad_f32(x):
    x = np.asarray(x, f32)
    cdf = f32(0.5) * (f32(1) + _erf64(x * f32(0.70710678118654752440)).astype(f32))
    pdf = f32(0.39894228040143267794) * _exp32(f32(-0.5) * x * x)
    return cdf + x * pdf


def quick_gelu_grad_f32(x):
    x = np.asarray(x, f32)
    s = (1.0 / (f32(1) + _exp32(f32(-1.702) * x)).astype(np.float64)).astype(f32)
    return s * (f32(1) + f32(1.702) * x * (f32(1) - s))


def act64(act, x):
    x = np.asarray(x, np.float64)
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + _erf64(x / math.sqrt(2.0)))
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-1.702 * x))


def grad64(act, x):
    x = np.asarray(x, np.float64)
    if act == ACT_GELU_BWD:
        return 0.5 * (1.0 + _erf64(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-1.702 * x))
    return s * (1.0 + 1.702 * x * (1.0 - s))


_MEASURED: Dict = {}


def measure_act_errors() -> Dict:
    """max |float32 restatement - float64| of the four functions over |x| <= ACT_RANGE (2^17 points, dense around 0, plus every bf16
    value in range: the aux operand is bf16).  ACT_ABS / GRAD_ABS of the bounds; the CPU test pins their ceilings."""
    if not _MEASURED:
        g = np.concatenate([np.linspace(-ACT_RANGE, ACT_RANGE, 1 << 16), np.linspace(-1, 1, 1 << 15), np.linspace(-1e-2, 1e-2, 1 << 14)]).astype(f32)
        b = bf16_f32(np.arange(65536, dtype=np.uint32).astype(np.uint16))
        b = b[np.isfinite(b) & (np.abs(b) <= ACT_RANGE)]
        _MEASURED[ACT_GELU] = float(np.max(np.abs(gelu_fast_f32(g).astype(np.float64) - act64(ACT_GELU, g))))
        _MEASURED[ACT_QUICK_GELU] = float(np.max(np.abs(quick_gelu_fast_f32(g).astype(np.float64) - act64(ACT_QUICK_GELU, g))))
        _MEASURED[ACT_GELU_BWD] = float(np.max(np.abs(gelu_grad_f32(b).astype(np.float64) - grad64(ACT_GELU_BWD, b))))
        _MEASURED[ACT_QUICK_GELU_BWD] = float(np.max(np.abs(quick_gelu_grad_f32(b).astype(np.float64) - grad64(ACT_QUICK_GELU_BWD, b))))
    return _MEASURED


def qgrad_bound(x) -> np.ndarray:
    """quick_gelu_grad_f = s (1 + 1.702 x (1 - s)), s = 1 / (1 + __expf(-1.702 x)) with HIP's fp32 division (2.5 ulp promised):
    m = fl(1.702 x); e = exp(-m): relative 2^-23 (1 + 2 |m|) (v_exp_f32 and the two roundings of its argument); d = fl(1 + e): U;
    ds = s [(1 - s)(1 + 2 |m|) 2^-23 + U + 2.5 x 2^-23] (d s / s = (1 - s) d e / e);  om = fl(1 - s): d_om = ds + U (1 - s);
    p = fl(fl(1.702 x) om): dp = |m| d_om + 2 U |p|;  q = fl(1 + p): dq = dp + U |q|;  g = fl(s q): dg = |q| ds + s dq + ds dq + U |g|;
    plus GRAD_ABS, the restatement's own measured roundings."""
    x = np.asarray(x, np.float64)
    m = 1.702 * x
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-m))
    ds = s * ((1.0 - s) * (1.0 + 2.0 * np.abs(m)) * HW_ULP + U + 2.5 * HW_ULP)
    d_om = ds + U * (1.0 - s)
    p = m * (1.0 - s)
    dp = np.abs(m) * d_om + 2.0 * U * np.abs(p)
    q = 1.0 + p
    dq = dp + U * np.abs(q)
    return np.abs(q) * ds + s * dq + ds * dq + U * np.abs(s * q) + measure_act_errors()[ACT_QUICK_GELU_BWD]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def _rng(c: Case, salt: int = 0):
    return np.random.default_rng([zlib.crc32(c.id.encode()), salt])


def _pad2(live: np.ndarray, ld: int, pre: int, post: int, fill) -> np.ndarray:
    """(pre + rows + post, ld) buffer filled with `fill`, `live` at rows pre.., columns 0.."""
    buf = np.full((pre + live.shape[0] + post, ld), fill, dtype=live.dtype)
    buf[pre:pre + live.shape[0], :live.shape[1]] = live
    return buf


def _vec(live: np.ndarray) -> np.ndarray:
    return np.concatenate([live.astype(f32), np.full(VEC_PAD, np.nan, f32)])


def _quarter_ints(rng, shape, lim=8):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64) / 4.0


def _distinct_rows(a: np.ndarray, what: str, c: Case):
    assert np.unique(np.ascontiguousarray(a), axis=0).shape[0] == a.shape[0], (c.id, what, "two equal rows")


def _partials(x64: np.ndarray, parts: int) -> np.ndarray:
    """(rows, parts, 2) fp32 {sum, sum of squares} of `parts` column slices of the rows"""
    rows, width = x64.shape
    cuts = np.linspace(0, width, parts + 1).astype(int)
    out = np.zeros((rows, parts, 2), np.float64)
    for p in range(parts):
        seg = x64[:, cuts[p]:cuts[p + 1]]
        out[:, p, 0] = seg.sum(1)
        out[:, p, 1] = (seg * seg).sum(1)
    return out.astype(f32)


def make(c: Case) -> Dict:
    """Every buffer of the launch as the kernel sees it: inputs with NaN pads and rows behind, outputs filled with sentinels.  `pre`
    gives the rows in front of each buffer's row 0."""
    rng = _rng(c)
    M, N, K = c.M, c.N, c.K
    exact = c.family == "exact"
    inp: Dict = {"pre": {}}
    if exact:
        A, W = _quarter_ints(rng, (M, K)), _quarter_ints(rng, (N, K))
        if M <= 4096:
            _distinct_rows(A, "A", c)
        _distinct_rows(W, "W", c)
    else:
        A = rng.standard_normal((M, K))
        if c.ln == "fold":
            A = A + rng.uniform(-1.0, 1.0, (M, 1)) + 0.25      # rows with a non-zero mean (|mean| / std <= 1.25: the trained streams' range)
        W = rng.standard_normal((N, K)) / math.sqrt(K)
    Ab, Wb = bf16_bits(A.astype(f32)), bf16_bits(W.astype(f32))
    inp["A"], inp["W"] = _pad2(Ab, c.lda, 0, POST, NAN_BF16), _pad2(Wb, c.ldw, 0, POST, NAN_BF16)
    if c.bias:
        b = (np.arange(N) - N // 2) / 16.0 if exact else rng.standard_normal(N)
        inp["bias"] = _vec(b)
    if c.res != "none":
        if exact:
            r = rng.integers(-2 ** 14, 2 ** 14, size=(M, N)).astype(np.float64) / 16.0
            if c.res == "bf16":
                r = rng.integers(-128, 128, size=(M, N)).astype(np.float64) / 16.0      # 8 significant bits
        else:
            r = rng.standard_normal((M, N)) * 1.5 + 0.5
        r32 = r.astype(f32)
        if c.res == "f32":
            inp["res"] = _pad2(r32, c.ldr, 0, POST, f32(np.nan))
        elif c.res == "bf16":
            inp["resb"] = _pad2(bf16_bits(r32), c.ldrb, 0, POST, NAN_BF16)
        if c.ln == "rln":
            inp["r_stats"] = np.concatenate([_partials(r32.astype(np.float64), c.parts), np.full((POST, c.parts, 2), np.nan, f32)])
            inp["gamma"], inp["beta"] = _vec(1.0 + 0.25 * rng.standard_normal(N)), _vec(0.25 * rng.standard_normal(N))
    if c.ln == "fold":
        st = _partials(A if not exact else bf16_f32(Ab).astype(np.float64), c.parts)
        if c.guard == "nan":
            st[M // 2, 1, 0] = np.nan
        inp["a_stats"] = np.concatenate([st, np.full((POST, c.parts, 2), np.nan, f32)])
        inp["colsum"] = _vec(bf16_f32(Wb).astype(np.float64).sum(1))
    if c.act in (ACT_GELU_BWD, ACT_QUICK_GELU_BWD):
        inp["aux"] = _pad2(bf16_bits(np.clip(rng.standard_normal((M, N)) * 2.0, -8.0, 8.0).astype(f32)), c.ldaux, 0, POST, NAN_BF16)
    # outputs
    if c.outs in ("f32", "both"):
        if c.res == "inplace":
            inp["of"] = _pad2(r32, c.ldf, PRE, POST, SENT_F32)      # (its pads are sentinels, not NaN: the buffer is an output too)
        else:
            inp["of"] = np.full((PRE + M + POST, c.ldf), SENT_F32, f32)
        inp["pre"]["of"] = PRE
    if c.outs in ("bf16", "both"):
        inp["ob"] = np.full((PRE + M + POST, c.ldo), SENT_BF16, np.uint16)
        inp["pre"]["ob"] = PRE
    if c.out_stats:
        inp["ostats"] = np.full((PRE + M + POST, (N // 32) * 2), SENT_F32, f32)
        inp["pre"]["ostats"] = PRE
    if c.guard != "no":
        inp["guard"] = np.zeros(GUARD_SLOTS, f32)
    if exact and c.res in ("f32", "inplace") and M <= 4096:
        _distinct_rows(r32, "residual", c)
    return inp


def _live(buf, pre, rows, cols):
    return buf[pre:pre + rows, :cols]


def _residual64(c: Case, inp) -> Optional[np.ndarray]:
    if c.res == "f32":
        return _live(inp["res"], 0, c.M, c.N).astype(np.float64)
    if c.res == "inplace":
        return _live(inp["of"], PRE, c.M, c.N).astype(np.float64)
    if c.res == "bf16":
        return bf16_f32(_live(inp["resb"], 0, c.M, c.N)).astype(np.float64)
    return None


def _row_stats(stats: np.ndarray, width: int, eps: float):
    """float64 mean, rstd of every row from its fp32 partials (rows, P, 2) and the bounds d_mean, d_rstd of the kernel's fp32 ones"""
    s = stats.astype(np.float64)
    P = s.shape[1]
    inv_h = float(f32(1.0) / f32(width))
    sm, sq = s[:, :, 0].sum(1), s[:, :, 1].sum(1)
    d_sm, d_sq = P * U * np.abs(s[:, :, 0]).sum(1), P * U * np.abs(s[:, :, 1]).sum(1)
    mean = sm * inv_h
    d_mean = d_sm * inv_h + U * np.abs(mean)
    raw = sq * inv_h - mean * mean
    var = np.maximum(raw, 0.0)
    d_var = d_sq * inv_h + U * np.abs(sq * inv_h) + 2 * np.abs(mean) * d_mean + d_mean ** 2 + U * np.abs(raw)
    ve = var + float(f32(eps))
    rstd = 1.0 / np.sqrt(ve)
    d_rstd = rstd * ((d_var + U * ve) / (2.0 * np.maximum(ve - d_var - U * ve, 1e-300)) + HW_ULP + U)
    return mean, rstd, d_mean, d_rstd


def row_stats(stats, width, eps):
    with np.errstate(invalid="ignore"):      # (a NaN statistic stays a NaN)
        return _row_stats(stats, width, eps)


BLAS32_FROM = 1 << 32            # multiply-adds from which the exact family's product is formed by an fp32 BLAS call
BLAS32_ROWS = 64                 # rows of that product that are compared with float64


def _product(c: Case, A: np.ndarray, W: np.ndarray) -> np.ndarray:
    """A W^T in float64.  In the exact family every partial sum of the K <= 768 products, in any order, is a multiple of 1/16 below
    4 K <= 3,072 (16 x 3,072 < 2^24): an fp32 product IS the float64 one, so the large cases (tests/gemm_pp_cases.py) take it from an
    fp32 BLAS call and compare a block of rows with float64."""
    if c.family != "exact" or c.M * c.N * c.K < BLAS32_FROM:
        return A @ W.T
    assert c.K <= 768
    acc = (A.astype(f32) @ W.astype(f32).T).astype(np.float64)
    r0 = (c.M // 2) // BLAS32_ROWS * BLAS32_ROWS
    for lo in (0, r0, c.M - BLAS32_ROWS):
        assert np.array_equal(acc[lo:lo + BLAS32_ROWS], A[lo:lo + BLAS32_ROWS] @ W.T), (c.id, "the fp32 product is not exact", lo)
    return acc


def reference(c: Case, inp: Dict) -> Dict:
    """name -> (reference, bound) over the LIVE region of each output: "of" / "ob" (M, N), "ostats" (M, N / 32, 2), "guard" scalar"""
    M, N, K = c.M, c.N, c.K
    A = bf16_f32(_live(inp["A"], 0, M, K)).astype(np.float64)
    W = bf16_f32(_live(inp["W"], 0, N, K)).astype(np.float64)
    acc = _product(c, A, W)
    exact = c.family == "exact"       # becomes False at the first operation that is not an exact add
    e = np.zeros_like(acc) if exact else ACC_ULP * K * (np.abs(A) @ np.abs(W).T)
    out: Dict = {}
    act_abs = measure_act_errors()
    if c.entry == "dgrad":
        v = acc
        if c.act != ACT_NONE:
            x = bf16_f32(_live(inp["aux"], 0, M, N)).astype(np.float64)
            assert np.abs(x).max() <= ACT_RANGE
            g = grad64(c.act, x)
            Eg = GELU_GRAD_HW + act_abs[ACT_GELU_BWD] if c.act == ACT_GELU_BWD else qgrad_bound(x)
            v = acc * g
            e = np.abs(g) * e + np.abs(acc) * Eg + e * Eg + U * np.abs(v)
            exact = False
        r = _residual64(c, inp)
        if r is not None:
            v = v + r
            e = e + (0.0 if exact else U * np.abs(v))
    else:
        v = acc
        mean = rstd = None
        if c.ln == "fold":
            mean, rstd, dm, dr = row_stats(inp["a_stats"][:M], K, EPS)
            cs = inp["colsum"][:N].astype(np.float64)
            t = acc - mean[:, None] * cs[None, :]
            e_t = e + dm[:, None] * np.abs(cs)[None, :] + U * np.abs(t)
            v = rstd[:, None] * t
            e = dr[:, None] * np.abs(t) + rstd[:, None] * e_t + dr[:, None] * e_t + U * np.abs(v)
            exact = False
            ratio = np.abs(mean) * rstd
            d_ratio = dm * rstd + np.abs(mean) * dr + dm * dr + U * ratio
            if c.guard != "no":
                if np.isnan(ratio).any():
                    out["guard"] = (np.array(np.inf), np.array(0.0))
                else:
                    out["guard"] = (np.array(ratio.max()), np.array(d_ratio.max()))
        if c.bias:
            v = v + inp["bias"][:N].astype(np.float64)[None, :]
            e = e + (0.0 if exact else U * np.abs(v))
        if c.act != ACT_NONE:
            with np.errstate(invalid="ignore"):
                assert np.nanmax(np.abs(v)) <= ACT_RANGE, (c.id, np.nanmax(np.abs(v)))
            y = act64(c.act, v)
            e = ACT_SLOPE * e + act_abs[c.act] + ACT_HW[c.act] * np.abs(v) + U * np.abs(y)
            v = y
            exact = False
        r = _residual64(c, inp)
        if r is not None:
            e_r = 0.0
            if c.ln == "rln":
                mean, rstd, dm, dr = row_stats(inp["r_stats"][:M], N, EPS)
                gm, bt = inp["gamma"][:N].astype(np.float64)[None, :], inp["beta"][:N].astype(np.float64)[None, :]
                d0 = r - mean[:, None]
                e1 = dm[:, None] + U * np.abs(d0)
                n0 = d0 * rstd[:, None]
                e2 = np.abs(d0) * dr[:, None] + rstd[:, None] * e1 + dr[:, None] * e1 + U * np.abs(n0)
                r = n0 * gm + bt
                e_r = np.abs(gm) * e2 + U * np.abs(r)
                exact = False
            v = v + r
            e = e + e_r + (0.0 if exact else U * np.abs(v))
    nan = np.isnan(v)
    e = np.where(nan, 1.0, e)
    if c.outs in ("f32", "both"):
        out["of"] = (v, e)
    if c.outs in ("bf16", "both"):
        out["ob"] = (v, e)          # (compared by bf16_ratio)
    if c.out_stats:
        g = v.reshape(M, N // 32, 32)
        ge = np.broadcast_to(e, v.shape).reshape(M, N // 32, 32)
        ref = np.stack([g.sum(2), (g * g).sum(2)], axis=2)
        bnd = np.stack([ge.sum(2) + 32 * U * np.abs(g).sum(2), (2 * np.abs(g) * ge + ge * ge).sum(2) + 33 * U * (g * g).sum(2)], axis=2)
        out["ostats"] = (ref, bnd)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparison of whole buffers
def _sentinel_ok(buf: np.ndarray, pre: int, rows: int, cols: int, sent) -> bool:
    mask = np.ones(buf.shape, bool)
    mask[pre:pre + rows, :cols] = False
    return bool((buf[mask] == sent).all())


def bf16_ratio(got, ref, e) -> float:
    """max over the elements of (distance from ref to the nearest real that rounds to got) / e; inf where e = 0 and got is not the
    round-to-nearest-even of ref, or where a NaN is on one side only.  The reals that round to a bf16 value g (ties aside) are the
    interval between its midpoints with its two neighbours."""
    got, ref, e = (np.asarray(a, np.float64) for a in (got, ref, e))
    gn, rn = np.isnan(got), np.isnan(ref)
    if (gn != rn).any():
        return math.inf
    ok = ~rn
    g, r = np.where(ok, got, 0.0), np.where(ok, ref, 0.0)
    same = bf16_round(r.astype(f32)).astype(np.float64) == g
    sel = ~same & ok                                                        # (only these have a distance: the rest is RNE(ref) itself)
    if not sel.any():
        return 0.0
    e = np.broadcast_to(e, g.shape)
    g, r, e, ok, same = g[sel], r[sel], e[sel], ok[sel], same[sel]
    mag = np.abs(g)
    ulp = bf16_ulp(mag)                                                     # spacing above |g|
    below = np.where(mag == 2.0 ** np.floor(np.log2(np.where(mag > 0, mag, 1.0))), ulp / 2, ulp)      # spacing below (a power of two: half)
    lo, hi = mag - below / 2, mag + ulp / 2                                 # |x| that round to |g|
    rs = np.where(g != 0, r * np.sign(g), np.abs(r))                        # ref on g's side of zero (negative: the sign differs)
    dist = np.where(rs < lo, lo - rs, np.where(rs > hi, rs - hi, 0.0))
    dist = np.where(same | ~ok, 0.0, dist)
    if (dist[e == 0] != 0).any() or (~same & (e == 0) & ok).any():
        return math.inf
    nz = (e > 0) & ok
    return float(np.max(dist[nz] / e[nz])) if nz.any() else 0.0


def check(c: Case, inp: Dict, got: Dict, refs: Optional[Dict] = None, cus: Optional[int] = None) -> Dict[str, float]:
    """name -> worst |got - ref| / bound over the live region (inf: a bit differs where the bound is 0, a NaN on one side, or a
    sentinel was overwritten).  `got` holds whole buffers, laid out as make()'s.  `cus`: the device's CU count (the persistent
    form's grid, i.e. the guard slots its workgroups own)."""
    refs = reference(c, inp) if refs is None else refs
    out = {}
    for name, (ref, bnd) in refs.items():
        if name == "guard":
            g = got["guard"]
            grid = planned_grid(c, cus)
            r = worst_ratio(np.array(float(g.max()) if not np.isnan(g).any() else np.nan), ref, bnd)
            if (g[min(grid, GUARD_SLOTS):] != 0).any() or (g < 0).any():
                r = math.inf           # a slot no workgroup owns was written
            out[name] = r
            continue
        buf = got[name]
        cols = c.N if name != "ostats" else (c.N // 32) * 2
        sent = SENT_BF16 if name == "ob" else SENT_F32
        live = _live(buf, PRE, c.M, cols)
        val = bf16_f32(live) if name == "ob" else live
        r = bf16_ratio(val, ref, bnd) if name == "ob" else worst_ratio(val.reshape(ref.shape), ref, bnd)
        if not _sentinel_ok(buf, PRE, c.M, cols, sent):
            r = math.inf
        out[name] = r
    return out


def unequal(c: Case, got: Dict, refs: Dict) -> int:
    """elements of the fp32 / bf16 outputs that differ from the reference (the exact family's count)"""
    n = 0
    for name in ("of", "ob"):
        if name in refs:
            live = _live(got[name], PRE, c.M, c.N)
            val = bf16_f32(live) if name == "ob" else live
            want = bf16_round(refs[name][0].astype(f32)) if name == "ob" else refs[name][0]
            n += int((val.astype(np.float64) != want).sum())
    return n


def is_bit_exact(c: Case) -> bool:
    """cases whose fp32 / bf16 outputs carry the bound 0"""
    return c.family == "exact" and c.act == ACT_NONE and c.ln in ("none", "plain")


def grid_of(tile: int, M: int, N: int):
    bm, bn = tile_dims(tile)[:2]
    return (M + bm - 1) // bm, N // bn


def planned_grid(c: Case, cus: Optional[int] = None) -> int:
    """workgroups of the launch (each owns guard slot blockIdx.x % GUARD_SLOTS)"""
    m, n = grid_of(tile_of(c), c.M, c.N)
    if tile_of(c) == PP_TILE:
        return min(cus or PP_CUS, m * n) & ~7
    return m * n


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatement of the kernel (the epilogue's operation order; fp32 accumulation over 32-k halves in two orders) and the mutants
MUTANTS = ("last_k_half_dropped", "k_step_repeated_instead_of_last", "bias_one_column_right", "residual_read_with_ldf", "ldo_ldf_exchanged",
           "two_tiles_swapped", "one_tile_computed_twice", "mean_colsum_omitted", "r_gamma_beta_shifted_8", "partial_beyond_count_not_zeroed",
           "out_stats_group_off_by_one", "gelu_quick_gelu_exchanged", "act_grad_at_output")


def _stats32(stats: np.ndarray, width: int, eps: float, mutant=None):
    """the canonical order: 16-B chunk q (two partials) belongs to group q % 4, a group adds its chunks ascending, (g0 + g1) + (g2 + g3)"""
    rows, P, _ = stats.shape
    ch = stats.reshape(rows, P // 2, 4)
    nq = P // 2
    gs, gq = [], []
    for g in range(4):
        s = q = None
        for u in range(3):
            k = g + 4 * u
            if k < nq:
                x = ch[:, k]
            elif mutant == "partial_beyond_count_not_zeroed":
                x = ch[:, 0]            # the clamped load's value, not masked
            else:
                x = np.zeros((rows, 4), f32)
            s_, q_ = x[:, 0] + x[:, 2], x[:, 1] + x[:, 3]
            s, q = (s_, q_) if s is None else (s + s_, q + q_)
        gs.append(s)
        gq.append(q)
    sm, sq = (gs[0] + gs[1]) + (gs[2] + gs[3]), (gq[0] + gq[1]) + (gq[2] + gq[3])
    inv_h = f32(1.0) / f32(width)
    mean = sm * inv_h
    with np.errstate(invalid="ignore"):
        var = np.maximum(_fma(-mean, mean, sq * inv_h), f32(0))
        var = np.where(np.isnan(mean), f32(np.nan), var)
        rstd = (1.0 / np.sqrt((var + f32(eps)).astype(np.float64))).astype(f32)
    return mean.astype(f32), rstd


def _flat_load(buf: np.ndarray, pre: int, ld_buf: int, ld_used: int, rows: int, cols: int, shift: int = 0) -> np.ndarray:
    flat = buf.ravel()
    idx = pre * ld_buf + np.arange(rows)[:, None] * ld_used + np.arange(cols)[None, :] + shift
    return flat[np.clip(idx, 0, flat.size - 1)]


def _flat_store(buf: np.ndarray, pre: int, ld_buf: int, ld_used: int, val: np.ndarray, keep=None):
    flat = buf.ravel()
    rows, cols = val.shape
    idx = pre * ld_buf + np.arange(rows)[:, None] * ld_used + np.arange(cols)[None, :]
    ok = idx < flat.size
    if keep is not None:
        ok &= keep
    flat[idx[ok]] = val[ok]


def emulate(c: Case, inp: Dict, order: int = 0, mutant: Optional[str] = None) -> Dict:
    """the launch on copies of make()'s output buffers, in float32"""
    M, N, K = c.M, c.N, c.K
    A = bf16_f32(_live(inp["A"], 0, M, K))
    W = bf16_f32(_live(inp["W"], 0, N, K))
    halves = [(k, k + 32) for k in range(0, K, 32)]
    if mutant == "last_k_half_dropped":
        halves = halves[:-1]
    if mutant == "k_step_repeated_instead_of_last" and K >= 128:
        halves = halves[:-2] + halves[-4:-2]
    if order:
        halves = halves[::-1]
    acc = np.zeros((M, N), f32)
    for k0, k1 in halves:
        a, w = (A[:, k0:k1], W[:, k0:k1]) if not order else (A[:, k0:k1][:, ::-1], W[:, k0:k1][:, ::-1])
        acc = acc + (a @ w.T).astype(f32)
    got = {k: inp[k].copy() for k in ("of", "ob", "ostats", "guard") if k in inp}
    res = None
    if c.res in ("f32", "inplace"):
        src, pre, ldb = (inp["res"], 0, c.ldr) if c.res == "f32" else (inp["of"], PRE, c.ldf)
        used = c.ldf if mutant == "residual_read_with_ldf" and c.ldf != c.ldr else c.ldr
        res = _flat_load(src, pre, ldb, used, M, N)
    elif c.res == "bf16":
        res = bf16_f32(_live(inp["resb"], 0, M, N))
    with np.errstate(invalid="ignore", over="ignore"):
        if c.entry == "dgrad":
            v = acc
            if c.act != ACT_NONE:
                x = acc if mutant == "act_grad_at_output" else bf16_f32(_live(inp["aux"], 0, M, N))
                v = acc * (gelu_grad_f32(x) if c.act == ACT_GELU_BWD else quick_gelu_grad_f32(x))
            elif res is not None:
                v = acc + res
        else:
            v = acc
            if c.ln == "fold":
                mean, rstd = _stats32(inp["a_stats"][:M], K, EPS, mutant)
                cs = inp["colsum"][:N]
                t = acc if mutant == "mean_colsum_omitted" else _fma(-mean[:, None], cs[None, :], acc)
                v = rstd[:, None] * t
                if "guard" in got:
                    ratio = np.abs(mean) * rstd
                    ratio = np.where(np.isnan(ratio), f32(np.inf), ratio)
                    bm = tile_dims(tile_of(c))[0]
                    mt, nt = grid_of(tile_of(c), M, N)
                    slots = min(GUARD_SLOTS, planned_grid(c))      # (the persistent form: G workgroups share the tiles)
                    for b in range(mt * nt):      # (which row tile a workgroup id owns does not matter to the maximum over the slots)
                        tm = b // nt
                        got["guard"][b % slots] = max(got["guard"][b % slots], ratio[tm * bm:(tm + 1) * bm].max())
            if c.bias:
                v = v + _flat_load(inp["bias"][None, :], 0, 0, 0, 1, N, shift=1 if mutant == "bias_one_column_right" else 0)
            act = c.act
            if mutant == "gelu_quick_gelu_exchanged" and act:
                act = 3 - act
            if act == ACT_GELU:
                v = gelu_fast_f32(v)
            elif act == ACT_QUICK_GELU:
                v = quick_gelu_fast_f32(v)
            if res is not None:
                if c.ln == "rln":
                    mean, rstd = _stats32(inp["r_stats"][:M], N, EPS, mutant)
                    sh = 8 if mutant == "r_gamma_beta_shifted_8" else 0
                    gm, bt = _flat_load(inp["gamma"][None, :], 0, 0, 0, 1, N, sh), _flat_load(inp["beta"][None, :], 0, 0, 0, 1, N, sh)
                    res = _fma((res - mean[:, None]) * rstd[:, None], gm, bt)
                v = v + res
    v = v.astype(f32)
    keep = None
    if mutant in ("two_tiles_swapped", "one_tile_computed_twice"):
        bm, bn = tile_dims(tile_of(c))[:2]
        rows = min(bm, M)
        if mutant == "two_tiles_swapped":
            v = v.copy()
            a, b = v[:rows, :bn].copy(), v[:rows, bn:2 * bn].copy()
            v[:rows, :bn], v[:rows, bn:2 * bn] = b, a
        else:
            keep = np.ones((M, N), bool)
            keep[:rows, N - bn:] = False          # the last column tile of row tile 0 is never written
    ldo, ldf = (c.ldf, c.ldo) if mutant == "ldo_ldf_exchanged" else (c.ldo, c.ldf)
    if "of" in got:
        _flat_store(got["of"], PRE, c.ldf, ldf, v, keep)
    if "ob" in got:
        _flat_store(got["ob"], PRE, c.ldo, ldo, bf16_bits(v), keep)
    if "ostats" in got:
        g = v.reshape(M, N // 32, 4, 8)
        sm, sq = np.zeros(g.shape[:3], f32), np.zeros(g.shape[:3], f32)
        for q in range(8):
            sm = sm + g[..., q]
            sq = _fma(g[..., q], g[..., q], sq)
        sm = (sm[..., 0] + sm[..., 1]) + (sm[..., 2] + sm[..., 3])
        sq = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
        st = np.stack([sm, sq], axis=2).reshape(M, -1)
        if mutant == "out_stats_group_off_by_one":
            flat = got["ostats"].ravel()
            idx = PRE * st.shape[1] + np.arange(M)[:, None] * st.shape[1] + np.arange(st.shape[1])[None, :] + 2
            flat[idx] = st
        else:
            _flat_store(got["ostats"], PRE, st.shape[1], st.shape[1], st)
    return got


# which case kills which mutant (tests/test_gemm_bf16_cases.py asserts each pair; ids are built by _mk)
def _find(**kw) -> str:
    for c in CASES:
        if all(getattr(c, k) == v for k, v in kw.items()) and not c.refuse:
            return c.id
    raise KeyError(kw)


KILLS = {
    "last_k_half_dropped": _find(entry="ex", tile=22, K=64, family="exact"),
    "k_step_repeated_instead_of_last": _find(entry="ex", tile=22, K=192, family="exact"),
    "bias_one_column_right": _find(entry="gemm", family="exact", bias=True, res="f32", outs="both"),
    "residual_read_with_ldf": _find(entry="ex", tile=16, M=127, family="exact"),
    "ldo_ldf_exchanged": _find(entry="ex", tile=17, M=127, family="exact"),
    "two_tiles_swapped": _find(entry="ex", tile=2, M=3 * 256 + 5, family="exact"),
    "one_tile_computed_twice": _find(entry="ex", tile=8, M=3 * 256 + 5, family="exact"),
    "mean_colsum_omitted": _find(entry="ln", tile=20, ln="fold", family="rounded", act=0, parts=10, guard="no"),
    "r_gamma_beta_shifted_8": _find(entry="ln", tile=28, ln="rln", family="rounded", res="f32", parts=12, out_stats=False),
    "partial_beyond_count_not_zeroed": _find(entry="ln", tile=20, ln="fold", family="rounded", act=0, parts=22, guard="no"),
    "out_stats_group_off_by_one": _find(entry="ln", tile=17, ln="rln", family="rounded", res="bf16", parts=2, out_stats=True),
    "gelu_quick_gelu_exchanged": _find(entry="gemm", family="rounded", act=1, bias=True, res="none", outs="f32"),
    "act_grad_at_output": _find(entry="dgrad", family="rounded", act=ACT_GELU_BWD, outs="f32", N=128),
}
assert set(KILLS) == set(MUTANTS)
