"""The one-tile bf16 GEMM (csrc/gemm_bf16_kernel.hpp), op by op through the C ABI: every case of tests/gemm_bf16_cases.py -- one
launch of ufnd_gemm_bf16, ufnd_gemm_bf16_ex, ufnd_gemm_bf16_ln or ufnd_gemm_bf16_dgrad -- against the float64 reference and the
derived per-element bounds of that file (the derivations, the two data families, the poison and the sentinels are described there;
tests/test_gemm_bf16_cases.py shows on the CPU that the table reaches every tile, ring depth and grid form it claims and that the
bounds reject thirteen wrong kernels).

Inputs carry NaN in their pad columns and in the rows behind them, outputs a sentinel in their pad columns and in the rows in front
of and behind the M rows; G.check() returns inf for a damaged sentinel.  Each test prints its worst error / bound and, for the exact
family, the number of unequal elements; tools/gemm_bf16_errors.py collects them into profiles/gemm_bf16_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_bf16_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


def _dev(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def _host(t: torch.Tensor) -> np.ndarray:
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def launch(c: G.Case, inp: dict, m_live=None):
    """(return code, error text, {output name: whole buffer after the launch}).  m_live: a row count that goes to the device and the
    "ex" / "ln" launch through ufnd_gemm_bf16_live / ufnd_gemm_bf16_ln_live (tests/test_gpu_gemm_pp_cases.py)."""
    L = _lib()
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    t = {k: _dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    live = None if m_live is None else torch.tensor([m_live], dtype=torch.int32, device=DEV)

    def p(name, ld=0):
        if name not in t:
            return None
        return t[name].data_ptr() + inp["pre"].get(name, 0) * ld * t[name].element_size()

    of, ob = p("of", c.ldf), p("ob", c.ldo)
    res = of if c.res == "inplace" else p("res")
    M, N, K = c.M, c.N, c.K
    if c.entry == "gemm":
        rc = lib.ufnd_gemm_bf16(p("A"), p("W"), p("bias"), res, ob, of, M, N, K, c.lda, c.ldw, c.ldr, c.ldo, c.ldf, c.act, s)
    elif c.entry == "ex" and live is not None:
        rc = lib.ufnd_gemm_bf16_live(p("A"), p("W"), p("bias"), res, ob, of, M, N, K, c.lda, c.ldw, c.ldr, c.ldo, c.ldf, c.act, c.tile,
                                     live.data_ptr(), s)
    elif c.entry == "ex":
        rc = lib.ufnd_gemm_bf16_ex(p("A"), p("W"), p("bias"), res, ob, of, M, N, K, c.lda, c.ldw, c.ldr, c.ldo, c.ldf, c.act, c.tile, s)
    elif c.entry == "ln":
        ln = L.GemmLn(a_stats=p("a_stats"), colsum=p("colsum"), r_stats=p("r_stats"), r_gamma=p("gamma"), r_beta=p("beta"),
                      out_stats=p("ostats", (N // 32) * 2), a_parts=c.parts if c.ln == "fold" else 0, r_parts=c.parts if c.ln == "rln" else 0,
                      a_eps=G.EPS, r_eps=G.EPS, width=K if c.ln == "fold" else N, tile_cfg=c.tile, residual_bf16=p("resb"), ldrb=c.ldrb,
                      guard=p("guard"))
        if live is not None:
            rc = lib.ufnd_gemm_bf16_ln_live(p("A"), p("W"), p("bias"), res, ob, of, M, N, K, c.lda, c.ldw, c.ldr, c.ldo, c.ldf, c.act, C.byref(ln),
                                            live.data_ptr(), s)
        else:
            rc = lib.ufnd_gemm_bf16_ln(p("A"), p("W"), p("bias"), res, ob, of, M, N, K, c.lda, c.ldw, c.ldr, c.ldo, c.ldf, c.act, C.byref(ln), s)
    else:
        rc = lib.ufnd_gemm_bf16_dgrad(p("A"), p("W"), res, p("aux"), ob, of, M, N, K, c.lda, c.ldw, c.ldr, c.ldaux, c.ldo, c.ldf, c.act, s)
    torch.cuda.synchronize()
    err = lib.ufnd_last_error().decode() if rc != 0 else ""
    return rc, err, {k: _host(t[k]) for k in ("of", "ob", "ostats", "guard") if k in t}


def measure(c: G.Case, inp=None, refs=None, cus=None, keep=None):
    """(worst error / bound, the output it is on, unequal elements or None outside the exact family) of one case on the GPU.  A caller
    that launches a case more than once passes its inputs and reference (neither is written to) and a dict `keep` that receives the
    output buffers; cus: the device's CU count (the persistent form's grid, G.check)."""
    inp = G.make(c) if inp is None else inp
    rc, err, got = launch(c, inp)
    if keep is not None:
        keep.update(got)
    if c.refuse:
        assert rc == 1 and c.refuse in err, (c.id, rc, err)
        for k, v in got.items():      # nothing was launched
            assert np.array_equal(v, inp[k], equal_nan=(v.dtype != np.uint16)), (c.id, k)
        return 0.0, "refused", None
    assert rc == 0, (c.id, rc, err)
    refs = G.reference(c, inp) if refs is None else refs
    ratios = G.check(c, inp, got, refs, cus)
    key = max(ratios, key=lambda k: ratios[k])
    return ratios[key], key, (G.unequal(c, got, refs) if G.is_bit_exact(c) else None)


def _run(c: G.Case):
    r, key, ne = measure(c)
    print(f"{c.id}: worst error / bound {r:.3g} ({key})" + ("" if ne is None else f"; unequal elements {ne}") + f"   [{c.edge}]")
    assert r <= 1.0, (c.id, r, key)
    assert ne in (None, 0), (c.id, ne)


def _of(entry):
    cs = [c for c in G.CASES if c.entry == entry]
    return dict(argvalues=cs, ids=[c.id for c in cs])


@pytest.mark.parametrize("case", **_of("gemm"))
def test_gemm_bf16_auto_against_float64(case):
    _run(case)


@pytest.mark.parametrize("case", **_of("ex"))
def test_gemm_bf16_ex_against_float64(case):
    _run(case)


@pytest.mark.parametrize("case", **_of("ln"))
def test_gemm_bf16_ln_against_float64(case):
    _run(case)


@pytest.mark.parametrize("case", **_of("dgrad"))
def test_gemm_bf16_dgrad_against_float64(case):
    _run(case)
