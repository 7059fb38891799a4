"""Case table, float64 reference, bounds, float32 restatement and mutants of ufnd_conv1d_rows_bf16 (csrc/gemm_bf16.hip): the one-tile
bf16 GEMM of tests/gemm_bf16_cases.py with an OVERLAPPING-row A operand -- output row r reads the lda-strided window
flat(A)[r lda : r lda + K], lda < K allowed.  The data families, the bounds (accumulation K 2^-23 sum |a w|, bias, the gelu_fast terms,
the bf16 interval rule), the bf16 helpers, the poison and the sentinels are those of that file and are imported from it.  Shared by
tests/test_conv_rows_cases.py (CPU) and tests/test_gpu_audio_ops.py (GPU: every case through the C ABI).  NumPy only.

The A operand is ONE flat buffer of exactly (M - 1) lda + K live elements -- what the header obliges the caller to hold -- followed
by NaN: a row clamp, a range clamp or a K loop that reaches one element further puts a NaN into the output.

  exact    operands are multiples of 1/4, K <= 320, no activation: bound 0 (gemm_bf16_cases' argument).  Every indexing concern lives
           here: the overlapping windows (asserted pairwise different in make()), lda < K, = K, > K, ragged row tiles, the 4-slot ring
           against nk = 5, the XCD column split on and off, the automatic tile choice on both sides of its 20 / 16 boundary.
  rounded  the product's own K / lda / N at a few hundred rows: one positional-conv group (K = 6144 on lda = 48), conv layers 1-4
           (K = 1536 on lda = 1024), layer 6 (K = lda = 1024)."""
from __future__ import annotations

import math
import zlib
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from tests import gemm_bf16_cases as G
from tests.gemm_bf16_cases import (ACC_ULP, ACT_GELU, ACT_HW, ACT_NONE, ACT_SLOPE, MUTANT_FACTOR, NAN_BF16, POST, PRE, SENT_BF16,  # noqa: F401
                                   SENT_F32, U, bf16_bits, bf16_f32, f32)

TAIL = 512                        # NaN elements behind the live part of A (a whole K step and more)


class Case(NamedTuple):
    id: str
    M: int
    N: int
    K: int
    lda: int
    family: str                   # exact | rounded
    want: int                     # the tile the automatic choice must reach (auto_cfg of a plain GEMM of the same M, N, K)
    xcd: int                      # xcd_cols the launch must run with (2: the grid's column split over the XCDs is on)
    bias: bool
    outs: str                     # bf16 | f32 | both
    act: int
    ldw: int
    ldo: int
    ldf: int
    edge: str


def _mk(M, N, K, lda, family="exact", *, want=20, xcd=1, bias=True, outs="both", act=ACT_NONE, wide=True, edge=""):
    ldw, ldo, ldf = (K + 16, N + 24, N + 28) if wide else (K, N, N)
    cid = "-".join(b for b in (f"t{want}", f"{M}x{N}x{K}", f"lda{lda}", family[0], f"a{act}" if act else "", "b" if bias else "nb", f"o{outs}",
                               "x2" if xcd == 2 else "", "wide" if wide else "tight") if b)
    return Case(cid, M, N, K, lda, family, want, xcd, bias, outs, act, ldw, ldo, ldf, edge)


def _cases() -> List[Case]:
    out = []
    forms = [(True, "both", True), (False, "f32", True), (True, "bf16", False), (False, "both", True), (True, "f32", False)]      # rotate
    for i, M in enumerate((1, 127, 128, 129, 300)):
        bias, outs, wide = forms[i % len(forms)]
        out.append(_mk(M, 128, 192, 128, bias=bias, outs=outs, wide=wide, edge=f"kernel 3 stride 2 (windows overlap by 64), M={M} against bm=128"))
    out.append(_mk(130, 64, 128, 128, outs="bf16", bias=False, edge="kernel 2 stride 2: no overlap, lda = K"))
    out.append(_mk(257, 64, 64, 8, outs="f32", edge="the largest overlap: lda = 8"))
    out.append(_mk(70, 64, 320, 8, edge="the largest overlap, nk = 5 against the 4-slot ring"))
    out.append(_mk(263, 64, 192, 48, bias=False, edge="the positional conv's stride, lda = 48"))
    out.append(_mk(65, 64, 192, 256, outs="bf16", edge="lda > K, which the entry also accepts"))
    out.append(_mk(600, 512, 128, 64, xcd=2, edge="5 row tiles, 8 column tiles, 4 N > M: the XCD column split is on"))
    out.append(_mk(2100, 512, 128, 64, outs="f32", wide=False, edge="4 N < M: the XCD column split is off"))
    out.append(_mk(4736, 512, 128, 64, outs="bf16", bias=False, edge="37 x 4 = 148 tiles of 128 x 128: still tile 20"))
    out.append(_mk(4737, 512, 128, 64, want=16, outs="f32", edge="38 x 4 = 152: tile 16, its last row tile one row high"))
    out.append(_mk(4800, 512, 128, 64, want=16, wide=False, edge="tile 16, tight strides"))
    out.append(_mk(260, 64, 6144, 48, "rounded", act=ACT_GELU, outs="f32", edge="one positional-conv group"))
    out.append(_mk(200, 512, 1536, 1024, "rounded", act=ACT_GELU, outs="bf16", bias=False, edge="conv layers 1-4"))
    out.append(_mk(100, 512, 1024, 1024, "rounded", act=ACT_GELU, outs="f32", bias=False, edge="conv layer 6"))
    out.append(_mk(200, 512, 1536, 1024, "rounded", outs="both", edge="conv layers 1-4, no activation"))
    return out


CASES: List[Case] = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids collide"


def live_elements(c: Case) -> int:
    return (c.M - 1) * c.lda + c.K


def is_bit_exact(c: Case) -> bool:
    return c.family == "exact" and c.act == ACT_NONE


def windows(flat: np.ndarray, M: int, K: int, stride: int, last_row: Optional[int] = None) -> np.ndarray:
    """(M, K) rows flat[r stride : r stride + K]; indices past the buffer are clamped to its last element (a NaN)"""
    rows = np.minimum(np.arange(M), M - 1 if last_row is None else last_row)
    idx = rows[:, None] * stride + np.arange(K)[None, :]
    return flat[np.minimum(idx, flat.size - 1)]


def make(c: Case) -> Dict:
    rng = np.random.default_rng([zlib.crc32(c.id.encode()), 17])
    M, N, K = c.M, c.N, c.K
    n_live = live_elements(c)
    if c.family == "exact":
        assert K <= 320 and c.act == ACT_NONE
        a, W = G._quarter_ints(rng, n_live), G._quarter_ints(rng, (N, K))
    else:
        a, W = rng.standard_normal(n_live), rng.standard_normal((N, K)) / math.sqrt(K)
    inp: Dict = {"pre": {}}
    inp["A"] = np.concatenate([bf16_bits(a.astype(f32)), np.full(TAIL, NAN_BF16, np.uint16)])
    inp["W"] = G._pad2(bf16_bits(W.astype(f32)), c.ldw, 0, POST, NAN_BF16)
    if c.bias:
        inp["bias"] = G._vec((np.arange(N) - N // 2) / 16.0 if c.family == "exact" else rng.standard_normal(N))
    if c.family == "exact":      # a wrong row, a wrong window, a wrong weight row or a wrong bias entry is another value
        win = windows(inp["A"], M, K, c.lda)
        assert np.unique(win, axis=0).shape[0] == M, (c.id, "two equal windows")
        assert np.unique(inp["W"][:N, :K], axis=0).shape[0] == N, (c.id, "two equal rows of W")
        assert not c.bias or np.unique(inp["bias"][:N]).size == N
    if c.outs in ("f32", "both"):
        inp["of"] = np.full((PRE + M + POST, c.ldf), SENT_F32, f32)
        inp["pre"]["of"] = PRE
    if c.outs in ("bf16", "both"):
        inp["ob"] = np.full((PRE + M + POST, c.ldo), SENT_BF16, np.uint16)
        inp["pre"]["ob"] = PRE
    return inp


def epilogue_ref(acc, e, bias, act, exact):
    """gemm_bf16_cases.reference()'s plain epilogue on a float64 product `acc` carrying the bound `e`: bias (+ U |v| once something
    inexact has happened), the activation against the exact erf-GELU (slope 1.13 on the incoming error, ACT_ABS, ACT_HW |v|, U |y|)"""
    v = acc
    if bias is not None:
        v = v + bias[None, :]
        e = e + (0.0 if exact else U * np.abs(v))
    if act != ACT_NONE:
        assert np.abs(v).max() <= G.ACT_RANGE
        y = G.act64(act, v)
        e = ACT_SLOPE * e + G.measure_act_errors()[act] + ACT_HW[act] * np.abs(v) + U * np.abs(y)
        v = y
    return v, e


def reference(c: Case, inp: Dict) -> Dict:
    """name -> (reference, bound) over the (M, N) live region of "of" / "ob" ("ob" is judged by gemm_bf16_cases.bf16_ratio)"""
    A = bf16_f32(windows(inp["A"], c.M, c.K, c.lda)).astype(np.float64)
    W = bf16_f32(inp["W"][:c.N, :c.K]).astype(np.float64)
    assert not np.isnan(A).any()
    exact = c.family == "exact"
    acc = A @ W.T
    e = np.zeros_like(acc) if exact else ACC_ULP * c.K * (np.abs(A) @ np.abs(W).T)
    v, e = epilogue_ref(acc, e, inp["bias"][:c.N].astype(np.float64) if c.bias else None, c.act, exact)
    return {k: (v, e) for k, on in (("of", c.outs != "bf16"), ("ob", c.outs != "f32")) if on}


def check(c: Case, inp: Dict, got: Dict, refs: Optional[Dict] = None) -> Dict[str, float]:
    return G.check(c, inp, got, reference(c, inp) if refs is None else refs)


def unequal(c: Case, got: Dict, refs: Dict) -> int:
    return G.unequal(c, got, refs)


MUTANTS = ("rows_at_stride_K", "window_one_k_step_short", "range_clamp_sized_M_lda", "row_clamp_one_row_early")


def emulate(c: Case, inp: Dict, order: int = 0, mutant: Optional[str] = None) -> Dict:
    """the launch in float32 on copies of make()'s output buffers: fp32 accumulation over 32-k halves in two orders"""
    M, N, K = c.M, c.N, c.K
    stride = K if mutant == "rows_at_stride_K" else c.lda
    bits = windows(inp["A"], M, K, stride, last_row=M - 2 if mutant == "row_clamp_one_row_early" and M > 1 else None)
    A = bf16_f32(bits)
    if mutant == "range_clamp_sized_M_lda":      # a buffer-range clamp that believes the operand ends at M lda: what lies behind reads as zero
        idx = np.arange(M)[:, None] * stride + np.arange(K)[None, :]
        A = np.where(idx >= M * c.lda, f32(0), A)
    W = bf16_f32(inp["W"][:N, :K])
    halves = [(k, k + 32) for k in range(0, K, 32)]
    if mutant == "window_one_k_step_short":
        halves = halves[:-2]
    if order:
        halves = halves[::-1]
    acc = np.zeros((M, N), f32)
    with np.errstate(invalid="ignore"):
        for k0, k1 in halves:
            a, w = (A[:, k0:k1], W[:, k0:k1]) if not order else (A[:, k0:k1][:, ::-1], W[:, k0:k1][:, ::-1])
            acc = acc + (a @ w.T).astype(f32)
        v = acc + inp["bias"][None, :N] if c.bias else acc
        if c.act == ACT_GELU:
            v = G.gelu_fast_f32(v)
    v = v.astype(f32)
    got = {k: inp[k].copy() for k in ("of", "ob") if k in inp}
    if "of" in got:
        G._flat_store(got["of"], PRE, c.ldf, c.ldf, v)
    if "ob" in got:
        G._flat_store(got["ob"], PRE, c.ldo, c.ldo, bf16_bits(v))
    return got


def _find(**kw) -> str:
    return next(c.id for c in CASES if all(getattr(c, k) == v for k, v in kw.items()))


# which exact-family case breaks its equality under which mutant
KILLS = {
    "rows_at_stride_K": _find(M=129, K=192, lda=128),
    "window_one_k_step_short": _find(M=70, K=320, lda=8),
    "range_clamp_sized_M_lda": _find(M=263, lda=48),
    "row_clamp_one_row_early": _find(M=4737),
}
assert set(KILLS) == set(MUTANTS)
