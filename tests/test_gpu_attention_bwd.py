"""The attention backward (csrc/attention_bwd.hip) and the training forwards that feed it, case by case through the C ABI, against
the float64 references and derived bounds of tests/attention_bwd_cases.py (the cases, the derivations and the CPU evidence that
the bounds tell a wrong kernel from a rounded one are there and in tests/test_attention_bwd_cases.py).

A case runs ufnd_attention_bf16_lse[_dropout], then ufnd_attention_bf16_bwd[_dropout] on the ctx and lse it produced.  Every buffer is
carved out of a larger allocation: the inputs (qkv, dctx) have NaN rows in front of and behind them, the key mask has live words
around it, and ctx, lse, the workspace and dqkv are filled with NaN throughout -- an unwritten element of dqkv stays NaN and fails
the comparison, a write outside an output changes a sentinel, a read outside an input brings a NaN in.  Exact cases must have 0
unequal elements, rounded ones every element inside [RNE(ref - e), RNE(ref + e)].  Each test prints its worst error / allowance;
tools/attention_bwd_errors.py collects them into profiles/attention_bwd_errors.txt.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import attention_bwd_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRE, POST = 2, 3          # sentinel rows in front of and behind every buffer
NAN = float("nan")


def _L():
    from ultrafnd_git_amd import _lib as L
    return L


def _s():
    return _L().stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def _carve_bf16(bits=None, rows=0, cols=0):
    """(whole allocation, the carved rows): NaN everywhere, the carved rows = `bits` if given"""
    if bits is not None:
        rows, cols = bits.shape
    whole = torch.full((PRE + rows + POST, cols), NAN, dtype=torch.bfloat16, device=DEV)
    part = whole[PRE:PRE + rows]
    if bits is not None:
        part.copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16))
    return whole, part


def _carve_f32(n, cols=1):
    whole = torch.full((PRE + n + POST, cols), NAN, dtype=torch.float32, device=DEV)
    return whole, whole[PRE:PRE + n]


def _sentinels_intact(whole, rows):
    return bool(torch.isnan(whole[:PRE].float()).all()) and bool(torch.isnan(whole[PRE + rows:].float()).all())


def _values(part):
    """a carved bf16 block as float32 values"""
    return A.bf16_f32(part.contiguous().view(torch.int16).cpu().numpy().view(np.uint16))


def run_case(c, inp):
    """{ctx, lse, dqkv} of one case from the kernels; asserts the sentinels and that no input changed"""
    L = _L()
    lib = L.lib()
    B, Lq, heads = c.B, c.L, c.heads
    rows, H = B * Lq, heads * 64
    qkv_w, qkv = _carve_bf16(inp["qkv"])
    dctx_w, dctx = _carve_bf16(inp["dctx"])
    qkv0, dctx0 = qkv_w.view(torch.int16).clone(), dctx_w.view(torch.int16).clone()
    ctx_w, ctx = _carve_bf16(rows=rows, cols=H)
    dqkv_w, dqkv = _carve_bf16(rows=rows, cols=3 * H)
    lse_w, lse = _carve_f32(rows, heads)
    wsf = lib.ufnd_attention_bwd_workspace_floats(B, Lq, heads)
    assert wsf == rows * heads
    ws_w, ws = _carve_f32(wsf)
    mask_w = mask = None
    if inp["mask"] is not None:
        mask_w = torch.ones(PRE + rows + POST, dtype=torch.int32, device=DEV)
        mask = mask_w[PRE:PRE + rows]
        mask.copy_(torch.from_numpy(inp["mask"].reshape(-1)))
    if c.p > 0:
        from ultrafnd_git_amd.state import StepStateBuffer
        st = StepStateBuffer(torch.device(DEV, torch.cuda.current_device()), seed=A.DROP_SEED + Lq)
        st.set_u64("step", A.DROP_STEP)
        drop = L.Dropout(st.ptr, c.p, A.DROP_TAG)
        L.check(lib.ufnd_attention_bf16_lse_dropout(qkv.data_ptr(), L.ptr(mask), ctx.data_ptr(), lse.data_ptr(), B, Lq, heads, C.byref(drop), _s()),
                "ufnd_attention_bf16_lse_dropout")
        L.check(lib.ufnd_attention_bf16_bwd_dropout(qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), L.ptr(mask), dqkv.data_ptr(),
                                                    ws.data_ptr(), B, Lq, heads, C.byref(drop), _s()), "ufnd_attention_bf16_bwd_dropout")
    else:
        L.check(lib.ufnd_attention_bf16_lse(qkv.data_ptr(), L.ptr(mask), ctx.data_ptr(), lse.data_ptr(), B, Lq, heads, _s()), "ufnd_attention_bf16_lse")
        L.check(lib.ufnd_attention_bf16_bwd(qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), L.ptr(mask), dqkv.data_ptr(), ws.data_ptr(),
                                            B, Lq, heads, _s()), "ufnd_attention_bf16_bwd")
    torch.cuda.synchronize()
    for name, whole, n in (("ctx", ctx_w, rows), ("lse", lse_w, rows), ("dqkv", dqkv_w, rows), ("workspace", ws_w, wsf)):
        assert _sentinels_intact(whole, n), f"{name}: a sentinel row changed"
    assert torch.equal(qkv_w.view(torch.int16), qkv0) and torch.equal(dctx_w.view(torch.int16), dctx0), "an input changed"
    if mask_w is not None:
        assert bool((mask_w[:PRE] == 1).all()) and bool((mask_w[PRE + rows:] == 1).all()) and np.array_equal(mask.cpu().numpy(), inp["mask"].reshape(-1))
    assert not bool(torch.isnan(ws).any()), "delta: an unwritten word"
    return {"ctx": _values(ctx), "lse": lse.cpu().numpy(), "dqkv": _values(dqkv)}


@functools.lru_cache(maxsize=None)
def _inputs(i):
    return A.make(A.CASES[i])


@functools.lru_cache(maxsize=None)
def _refs(i):
    return A.reference(A.CASES[i], _inputs(i))


def measure(i):
    """{output: (worst error / allowance, elements outside)} of case i's kernels"""
    c = A.CASES[i]
    return A.check(c, run_case(c, _inputs(i)), _refs(i))


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=[A.case_id(c) for c in A.CASES])
def test_case_against_float64(i):
    c = A.CASES[i]
    res = measure(i)
    kind = "exact" if A.is_exact(c) else "rounded"
    print(f"{A.case_id(c)} ({kind}): " + ", ".join(f"{k} {r:.3g} ({n} outside)" for k, (r, n) in res.items()))
    for k, (r, n) in res.items():
        assert n == 0 and r <= 1.0, (A.case_id(c), kind, k, r, n)
