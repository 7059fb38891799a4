"""The persistent, software-pipelined bf16 GEMM (csrc/gemm_bf16_pp.hpp, tile id 64) through the C ABI against float64: every case of
tests/gemm_pp_cases.py -- one launch of ufnd_gemm_bf16_ex / ufnd_gemm_bf16_ln with the tile forced, or of their _live forms with a
row count on the device -- under the derived per-element bounds of tests/gemm_bf16_cases.py (the table, what each shape reaches and the
live-row rules are described in tests/gemm_pp_cases.py; tests/test_gemm_pp_cases.py shows on the CPU that the table reaches what it
claims and that the bounds reject eight wrong kernels).  The launch and the judgement are tests/test_gpu_gemm_bf16.py's.

Every case runs TWICE on fresh buffers -- operands with NaN in their pad columns and behind their last row, outputs full of
sentinels -- both runs are judged and must agree bit for bit (the kernel's vmcnt schedule is counted by hand: a race shows as two
different answers).  Each test prints its figures before it asserts; tools/gemm_pp_errors.py collects them into
profiles/gemm_pp_errors.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import gemm_bf16_cases as G
from tests import gemm_pp_cases as P
from tests import test_gpu_gemm_bf16 as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def cu_count() -> int:
    return int(_lib().lib().ufnd_device_cu_count())


@functools.lru_cache(maxsize=1)
def _made(cid: str):
    """inputs of a live case's launch, shared by its row counts (never written to: make_live copies what it poisons)"""
    return P.make(next(lc.case for lc in P.LIVE_CASES if lc.case.id == cid))


def _same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def _judge(c, inp, got, refs):
    ratios = P.check(c, inp, got, refs, cu_count())
    key = max(ratios, key=lambda k: ratios[k])
    return ratios[key], key, (P.unequal(c, got, refs) if P.is_bit_exact(c) else None)


def _report(cid, runs, same, edge):
    """runs: (worst error / bound, the output it is on, unequal elements or None) per launch; prints, then asserts"""
    for k, (r, key, ne) in enumerate(runs):
        print(f"{cid} run {k}: worst error / bound {r:.3g} ({key})" + ("" if ne is None else f"; unequal elements {ne}"))
    r, key, ne = max(runs, key=lambda x: (x[0], x[2] or 0))
    print(f"{cid}: worst error / bound {r:.3g} ({key})" + ("" if ne is None else f"; unequal elements {ne}") +
          f"; runs bit-equal {same}   [{edge}]")
    for r, key, ne in runs:
        assert r <= 1.0, (cid, r, key)
        assert ne in (None, 0), (cid, ne)
    assert same, (cid, "two launches of the same call differ")


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_persistent_gemm_against_float64(case):
    inp = P.make(case)
    refs = P.reference(case, inp)
    first = {}
    runs = [T.measure(case, inp, refs, cu_count(), first)]
    rc, err, second = T.launch(case, inp)
    assert rc == 0, (case.id, rc, err)
    same = _same(first, second)
    # (the judgement is a function of the bits: a second launch that left the same bits has the first one's figures)
    runs.append(runs[0] if same else _judge(case, inp, second, refs))
    _report(case.id, runs, same, case.edge)


@pytest.mark.parametrize("lc", P.LIVE_CASES, ids=[lc.id for lc in P.LIVE_CASES])
def test_persistent_gemm_live_rows_against_float64(lc):
    c = lc.case
    inp = P.make_live(lc, _made(c.id))
    refs = P.live_refs(lc, inp)
    runs, outs = [], []
    for _ in range(2):
        rc, err, got = T.launch(c, inp, m_live=lc.m_live)
        assert rc == 0, (lc.id, rc, err)
        if outs and _same(outs[0], got):
            runs.append(runs[0])
        else:
            ratios = P.check_live(lc, inp, got, cu_count(), refs)
            key = max(ratios, key=lambda k: ratios[k])
            runs.append((ratios[key], key, P.unequal_live(lc, got, refs) if P.is_bit_exact(c) else None))
        outs.append(got)
    _report(lc.id, runs, _same(*outs), f"{lc.live} live rows of {c.M}")


def test_the_table_still_covers_its_list_on_this_device():
    """the coverage list of tests/test_gemm_pp_cases.py, recomputed for the CU count of the device the cases run on"""
    gaps = P.coverage_gaps(P.CASES, P.LIVE_CASES, cu_count())
    print(f"{cu_count()} CUs: coverage gaps {gaps}")
    assert not gaps, f"on {cu_count()} CUs the table of tests/gemm_pp_cases.py no longer reaches: {gaps}"


@pytest.mark.parametrize("case", P.STAMP_CASES, ids=[c.id for c in P.STAMP_CASES])
def test_every_workgroup_walks_the_tiles_the_mirror_says(case):
    """the stamps build of the diagnostics library (dbg = 1) leaves each workgroup's tile count behind its stamps: per blockIdx.x it
    is walk()'s for this device, and the output of that build meets the case's bound.

    This test found a defect of the stamps build (gemm_pp_kernel<PLAIN, none, DBG = 1>; the product instantiations were right): on
    512 x 640, 224, 64, 64, 0 and 96 of 327,680 elements came out unequal in five launches, other ones every time, always the first two
    of a 16-B output chunk in a workgroup's last tile, while the product entry gave 0 on the same buffers.  Cause, read from the
    listing: `buffer_store_dwordx4 v[2:5] ..` directly followed by `v_add_f32 v2, ..` -- a VALU write to a wide store's data register
    in the next instruction, which the compiler leaves without a wait state when the store's offset is in an SGPR.  The stamps build now
    keeps the data registers alive for two wait states (slice_rows_c), and tools/audit_pp_asm.py refuses such a pair in the product
    listing (tests/test_pp_audit.py)."""
    from tools import _diaglib
    L = _lib()
    cus = cu_count()
    want = [len(mine) for mine in P.walk_of(case, cus)]
    g = len(want)
    inp = P.make(case)
    t = {k: T._dev(inp[k]) for k in ("A", "W", "bias", "ob")}
    stamps = torch.zeros(9 * max(g, 256), dtype=torch.int64, device=DEV)
    ob = t["ob"].data_ptr() + G.PRE * case.ldo * 2
    rc = _diaglib.diag().ufnd_diag_gemm_pp_stamps(t["A"].data_ptr(), t["W"].data_ptr(), ob, case.M, case.N, case.K, stamps.data_ptr(), None,
                                                  t["bias"].data_ptr(), case.act, 1, L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0, _diaglib.diag().ufnd_diag_last_error()
    counts = stamps.cpu().numpy()[8 * g:9 * g].tolist()
    refs = P.reference(case, inp)
    ratios = P.check(case, inp, {"ob": T._host(t["ob"])}, refs, cus)
    ne = P.unequal(case, {"ob": T._host(t["ob"])}, refs)
    print(f"{case.id}: {cus} CUs, {g} workgroups; tiles per workgroup {sorted(set(counts))} (mirror {sorted(set(want))}); "
          f"workgroups that differ {sum(a != b for a, b in zip(counts, want))}; worst error / bound {max(ratios.values()):.3g}; unequal elements {ne}")
    assert counts == want
    assert max(ratios.values()) <= 1.0 and ne == 0


def test_the_product_entry_refuses_an_output_that_reaches_2_31_bytes():
    """ufnd_gemm_bf16_ex, tile 64, 2048 x 128 with ldo = 524,800: the last row ends 2^31 + 1,047,808 bytes behind out_bf16.  The output is
    allocated at its full size (2.15 GB, never filled, never read back), so a launcher that lost the check would still write inside it."""
    L = _lib()
    M, N, K, ldo = 2048, 128, 768, 524800
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    W = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    out = torch.empty((M - 1) * ldo + N, dtype=torch.bfloat16, device=DEV)
    assert out.numel() * 2 >= 2 ** 31
    rc = L.lib().ufnd_gemm_bf16_ex(A.data_ptr(), W.data_ptr(), None, None, out.data_ptr(), None, M, N, K, K, K, 0, ldo, 0, 0, P.PP,
                                   L.stream_ptr(torch.device(DEV)))
    err = L.lib().ufnd_last_error().decode()
    torch.cuda.synchronize()
    print(f"rc {rc}: {err}")
    assert rc != 0 and "persistent form" in err and "out_bf16 reaches" in err and "2^31 bytes" in err, (rc, err)
    del out
    torch.cuda.empty_cache()
