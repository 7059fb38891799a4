"""CPU: the table of tests/conv_rows_cases.py (ufnd_conv1d_rows_bf16) reaches the tile and the grid split each case names, its bounds
accept a float32 restatement in two summation orders, and four wrong address rules break an exact equality.

ufnd_conv1d_rows_bf16 calls the same auto_cfg and xcd_cols_for as ufnd_gemm_bf16 with (M, N, K) alone, so the tile and xcd_cols of a
case are read from the diagnostics plan entry (no launch, no GPU) of a plain GEMM of the same M, N, K."""
import math

import numpy as np
import pytest

from tests import conv_rows_cases as R
from tests import gemm_bf16_cases as G


@pytest.fixture(scope="module")
def D():
    from tools import _diaglib
    _diaglib.diag()
    return _diaglib


def test_every_case_reaches_the_tile_and_grid_split_it_names(D):
    seen = set()
    for c in R.CASES:
        rc, p, err = D.gemm_bf16_plan("gemm", A=0x100000, W=0x200000, bias=0x300000 if c.bias else None, out_bf16=0x400000 if c.outs != "f32" else None,
                                      out_f32=0x500000 if c.outs != "bf16" else None, M=c.M, N=c.N, K=c.K, lda=c.K, ldw=c.ldw, ldo=c.ldo, ldf=c.ldf,
                                      act=c.act)
        assert rc == 0, (c.id, err)
        assert p["tile"] == c.want and p["xcd_cols"] == c.xcd, (c.id, p)
        assert (p["m_tiles"], p["n_tiles"]) == G.grid_of(c.want, c.M, c.N), (c.id, p)
        seen.add((p["tile"], p["xcd_cols"]))
    assert {(20, 1), (20, 2), (16, 1)} <= seen
    ex = [c for c in R.CASES if c.family == "exact"]
    assert {c.M for c in ex if (c.lda, c.K, c.N) == (128, 192, 128)} == {1, 127, 128, 129, 300}
    assert {c.outs for c in ex} == {"bf16", "f32", "both"} and {c.bias for c in ex} == {True, False}
    assert any(c.ldo > c.N and c.outs != "f32" for c in ex) and any(c.ldf > c.N and c.outs != "bf16" for c in ex)
    assert any(c.lda < c.K for c in ex) and any(c.lda == c.K for c in ex) and any(c.lda > c.K for c in ex)
    assert any(c.K // 64 == 5 and G.TILES[c.want][2] == 4 for c in ex)
    bm16 = G.TILES[16][0]
    assert any(c.want == 16 and c.M % bm16 == 1 for c in ex) and max(c.M * c.N * c.K for c in R.CASES) <= 4800 * 512 * 128
    rd = [c for c in R.CASES if c.family == "rounded"]
    assert {(c.K, c.lda, c.N) for c in rd} == {(6144, 48, 64), (1536, 1024, 512), (1024, 1024, 512)} and any(c.act == 0 for c in rd)


@pytest.fixture(scope="module")
def made():
    cache = {}

    def get(c):
        if c.id not in cache:
            inp = R.make(c)
            cache[c.id] = (inp, R.reference(c, inp))
        return cache[c.id]
    return get


def test_the_operand_is_exactly_as_long_as_the_header_obliges():
    for c in R.CASES:
        inp = R.make(c)
        a = G.bf16_f32(inp["A"])
        n = R.live_elements(c)
        assert not np.isnan(a[:n]).any() and np.isnan(a[n:]).all() and a.size == n + R.TAIL
        w = G.bf16_f32(inp["W"])
        assert np.isnan(w[:, c.K:]).all() and np.isnan(w[c.N:]).all()


def test_a_float32_restatement_stays_inside_every_bound(made):
    worst = (0.0, "-")
    for c in R.CASES:
        inp, refs = made(c)
        for order in (0, 1):
            got = R.emulate(c, inp, order)
            r = R.check(c, inp, got, refs)
            m = max(r.values())
            assert m <= 1.0, (c.id, order, r)
            if R.is_bit_exact(c):
                assert m == 0.0 and R.unequal(c, got, refs) == 0, (c.id, r)
            worst = max(worst, (m, c.id))
    print(f"conv_rows: worst error / bound of the restatement {worst[0]:.3g} at {worst[1]}")


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_wrong_address_rule_breaks_an_equality(mutant, made):
    c = R.BY_ID[R.KILLS[mutant]]
    assert R.is_bit_exact(c)
    inp, refs = made(c)
    r = R.check(c, inp, R.emulate(c, inp, 0, mutant), refs)
    print(f"{mutant}: error / bound {max(r.values()):.3g} at {c.id}")
    assert max(r.values()) == math.inf, (mutant, c.id, r)
