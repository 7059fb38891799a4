"""CPU: the case table of tests/test_gpu_gemm_pp_cases.py (tests/gemm_pp_cases.py: the persistent bf16 GEMM, tile id 64) reaches what
it claims, the launcher refuses what the kernel cannot address, and the bounds tell eight wrong kernels from a rounded one.

The mode, the tile counts, the grid G and the statistics partial count of every case, the automatic choice and every refusal are read
from the library's own host-side code (ufnd_diag_gemm_pp_plan: the product entries' argument checks, then pp_check_args, pp_pick and
the launch geometry, for a CU count given as an argument; no launch, no GPU).  The coverage list is computed from those answers and
P.walk(), the host mirror of the kernel's tile walk -- not from the case names."""
import math

import numpy as np
import pytest

from tests import gemm_bf16_cases as G
from tests import gemm_pp_cases as P
from tests.test_gemm_bf16_cases import plan_args

CUS = (64, 256, 304)


@pytest.fixture(scope="module")
def D():
    from tools import _diaglib
    _diaglib.diag()
    return _diaglib


def plan(D, c, cus=256, tile=P.PP, ln=None, **over):
    """the plan entry's answer for a case (with overrides of the arguments / of the ln fields)"""
    kw = plan_args(c, ln=ln or {}, **over)
    for k in ("aux", "ldaux", "tile"):
        kw.pop(k)
    return D.gemm_pp_plan(tile=tile, cus=cus, **kw)


@pytest.fixture(scope="module")
def plans(D):
    out = {}
    for c in P.CASES + [lc.case for lc in P.LIVE_CASES] + P.STAMP_CASES:
        for cus in CUS:
            rc, p, err = plan(D, c, cus)
            assert rc == 0, (c.id, cus, err)
            out[c.id, cus] = p
    return out


# ---------------------------------------------------------------------------------------------------------------------
def _shapes():
    s = {(c.M // P.BM, c.N // P.BN, None) for c in P.CASES + P.STAMP_CASES}
    s |= {(lc.case.M // P.BM, lc.case.N // P.BN, lc.m_live) for lc in P.LIVE_CASES}
    return sorted(s, key=lambda t: (t[0], t[1], -1 if t[2] is None else t[2]))


@pytest.mark.parametrize("cus", CUS)
def test_the_walk_deals_every_live_tile_exactly_once(cus):
    for m, n, live in _shapes():
        w = P.walk(m, n, cus, live)
        assert len(w) == P.grid(m, n, cus) and len(w) % 8 == 0 and len(w) >= 8
        live_m = m if live is None else (min(max(live, 0), m * P.BM) + P.BM - 1) // P.BM
        seen = sorted(t for mine in w for t in mine)
        assert seen == [(p, t) for p in range(live_m) for t in range(n)], (m, n, live, cus)


def test_the_walk_at_256_cus_is_what_the_table_says():
    want = {(1, 8): {1: 8}, (2, 4): {1: 8}, (2, 5): {1: 6, 2: 2}, (3, 5): {1: 1, 2: 7}, (5, 3): {1: 1, 2: 7}, (9, 1): {1: 7, 2: 1},
            (11, 24): {1: 248, 2: 8}, (32, 24): {3: 256}, (43, 24): {4: 248, 5: 8}}
    for (m, n), hist in want.items():
        got = {}
        for mine in P.walk(m, n, 256):
            got[len(mine)] = got.get(len(mine), 0) + 1
        assert got == hist, (m, n, got)
    assert {len(x) for x in P.walk(25, 24, 256)} == {2, 3} and {len(x) for x in P.walk(129, 6, 256)} == {3, 4}


def test_the_table_covers_the_list(plans):
    geo = {c.id: (plans[c.id, 256]["m_tiles"], plans[c.id, 256]["n_tiles"]) for c in P.CASES + [lc.case for lc in P.LIVE_CASES]}
    assert P.coverage_gaps(P.CASES, P.LIVE_CASES, 256, geo) == []
    assert P.coverage_gaps(P.CASES, P.LIVE_CASES, 256) == []


@pytest.mark.parametrize("drop,word", [
    (lambda c: c.M == 43 * 256, "second turn"),
    (lambda c: c.M == 43 * 256 or c.M == 129 * 256, "4 tiles"),
    (lambda c: (c.M // 256) % 4 != 0, "ragged row group"),
    (lambda c: P.mode_of(c) == "plain" and c.act == 1, "instantiation plain act 1"),
    (lambda c: P.mode_of(c) == "fold" and c.parts == 22, "a_parts 22"),
    (lambda c: P.mode_of(c) == "rln" and c.parts == 12, "r_parts 12"),
    (lambda c: P.mode_of(c) == "res" and not c.bias, "no bias in mode res"),
    (lambda c: c.M == 9 * 256 and c.lda == c.K, "tight strides at (9, 1)"),
    (lambda c: c.guard == "nan", "fold guard nan"),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else "")
def test_coverage_notices_a_removed_entry(drop, word):
    kept = [c for c in P.CASES if not drop(c)]
    assert len(kept) < len(P.CASES)
    gaps = P.coverage_gaps(kept, P.LIVE_CASES, 256)
    assert any(word in g for g in gaps), gaps


def test_coverage_needs_the_live_cases_for_an_idle_workgroup():
    assert any("0 tiles" in g for g in P.coverage_gaps(P.CASES, [], 256))


def test_the_plan_answers_what_the_table_claims(plans):
    for c in P.CASES + [lc.case for lc in P.LIVE_CASES] + P.STAMP_CASES:
        for cus in CUS:
            p = plans[c.id, cus]
            m, n = c.M // P.BM, c.N // P.BN
            assert P.MODES[p["mode"]] == P.mode_of(c) and p["act"] == c.act, (c.id, p)
            assert (p["m_tiles"], p["n_tiles"], p["pp_rows"]) == (m, n, P.PP_ROWS), (c.id, p)
            assert p["G"] == P.grid(m, n, cus) == G.planned_grid(c, cus), (c.id, cus, p)
            assert p["stat_parts"] == (c.N // 32 if c.out_stats else 0), (c.id, p)
            assert c.out_stats == (P.mode_of(c) in ("rln", "res")) and (not c.out_stats or G.has_stats_epilogue(P.PP, c.N))
            assert c.K == P.K and c.tile == P.PP and c.outs == "bf16" and c.res in ("none", "bf16")


def _rule(mode, act, M, N, cus):
    """pp_pick's documented rule"""
    tiles, g = (M // 256) * (N // 128), cus & ~7
    if mode == "fold" and act and tiles >= 512:
        return 1
    rounds = (tiles + g - 1) // g
    return int(tiles >= 3 * g and tiles * 100 >= rounds * g * 93)


@pytest.mark.parametrize("cus", CUS)
def test_the_automatic_choice_follows_its_rule(D, plans, cus):
    for m, n, act, want256 in ((32, 24, 1, 1), (16, 24, 1, 0), (64, 18, 0, 0)):      # 8192 x 3072, 4096 x 3072 fold + GELU, 16384 x 2304 fold
        c = P._pp("fold", m, n, "rounded", act=act, parts=24)
        rc, p, err = plan(D, c, cus, tile=-1)
        assert rc == 0 and p["picked"] == _rule("fold", act, c.M, c.N, cus), (c.id, cus, p, err)
        if cus == 256:
            assert p["picked"] == want256, (c.id, p)
    for c in P.CASES:      # a forced call reports what the automatic choice would have done, and both ways agree
        rc, p, _ = plan(D, c, cus, tile=-1)
        assert rc == 0 and p["picked"] == plans[c.id, cus]["picked"] == _rule(P.mode_of(c), c.act, c.M, c.N, cus), (c.id, cus, p)
    assert plan(D, P.BY_ID[next(i for i in P.BY_ID if "32x24" in i)], 256, tile=-1)[1]["picked"] == 1
    for m, n in ((96, 6), (128, 6)):      # 32,768 x 768: exactly 3 tiles per workgroup at 192 / 256 CUs
        c = P._pp("res", m, n, "exact")
        assert plan(D, c, cus, tile=-1)[1]["picked"] == _rule("res", 0, c.M, c.N, cus)


# ---------------------------------------------------------------------------------------------------------------------
PLAIN = P._pp("plain", 8, 1, "exact")            # 2048 x 128
FOLD = P._pp("fold", 2, 5, "exact", parts=24)
RES = P._pp("res", 8, 1, "exact")
RLN = P._pp("rln", 2, 4, "exact", parts=24)
REACH = "2^31 bytes"
BIG_LD = 524800                                   # (2047 x 524,800 + 128) x 2 B = 2^31 + 1,047,808: rows of a 2048-row operand
REFUSALS = [
    # (base case, argument overrides, ln overrides, words of the refusal)
    (PLAIN, dict(K=704, lda=712, ldw=720), {}, "needs K = 768"),
    (PLAIN, dict(M=300), {}, "M % 256 == 0"),
    (PLAIN, dict(N=192, ldo=216), {}, "N % 128 == 0"),
    (PLAIN, dict(M=256, N=896, ldo=920), {}, "7 tiles are too few"),
    (PLAIN, dict(residual=0x900000, ldr=128), {}, "persistent form): unsupported call"),
    (PLAIN, dict(out_f32=0x900000, ldf=128), {}, "persistent form): unsupported call"),
    (PLAIN, dict(out_f32=0x900000, ldf=128, out_bf16=None), {}, "persistent form): unsupported call"),
    (RES, dict(act=1), {}, "activation"),
    (RLN, dict(act=2), {}, "activation"),
    (RES, dict(N=1024, ldo=1024), dict(ldrb=1024), "persistent form): out_stats unsupported for this shape"),
    (RES, {}, dict(out_stats=0xD00008), "persistent form): out_stats unsupported for this shape"),
    (PLAIN, dict(ldo=BIG_LD), {}, "out_bf16 reaches"),
    (RES, {}, dict(ldrb=BIG_LD), "residual_bf16 reaches"),
    (PLAIN, dict(lda=BIG_LD), {}, "A reaches"),
    (PLAIN, dict(ldw=8454664), {}, "W reaches"),               # (127 x 8,454,664 + 768) x 2 B >= 2^31
    (P._pp("res", 8, 6, "exact"), dict(M=11184896), {}, "out_stats reaches"),      # 11,184,896 rows x 24 partials x 8 B >= 2^31
    (P._pp("fold", 2, 24, "exact", parts=24), dict(M=349696), {}, "out_bf16 reaches"),      # tight rows would do: 349,696 x 3072 x 2 B >= 2^31
]


@pytest.mark.parametrize("base,over,ln_over,words", REFUSALS, ids=[f"{i}-{w[-28:].replace(' ', '_')}" for i, (_, _, _, w) in enumerate(REFUSALS)])
def test_the_launcher_refuses(D, base, over, ln_over, words):
    rc, p, err = plan(D, base)
    assert rc == 0 and p["mode"] >= 0, err
    rc, _, err = plan(D, base, ln=ln_over, **over)
    assert rc == 1 and words in err, (rc, err)
    if "reaches" in words:
        assert REACH in err, err
        rc, p, err = plan(D, base, tile=-1, ln=ln_over, **over)      # the automatic choice: not picked, so a one-tile kernel runs
        assert rc == 0 and p["picked"] == 0 and p["mode"] == -1, (rc, p, err)


def test_a_reach_just_below_the_limit_is_planned(D):
    """the limit is on the operand's END: (2047 x ldo + 128) x 2 B < 2^31 up to ldo = 524,544 (a multiple of 8)"""
    ld = (2 ** 30 - 128) // 2047 // 8 * 8
    assert (2047 * ld + 128) * 2 < 2 ** 31 <= (2047 * (ld + 8) + 128) * 2
    assert plan(D, PLAIN, ldo=ld)[0] == 0 and plan(D, PLAIN, ldo=ld + 8)[0] == 1
    assert plan(D, PLAIN, lda=(2 ** 30 - 768) // 2047 // 8 * 8)[0] == 0
    rc, p, _ = plan(D, P._pp("fold", 64, 24, "rounded", act=1, parts=24), tile=-1)      # 16,384 x 3072 FFN1: far below, picked
    assert rc == 0 and p["picked"] == 1
    rc, p, _ = plan(D, P._pp("fold", 64, 24, "rounded", act=1, parts=24), tile=-1, M=349696)      # the same Linear past the limit
    assert rc == 0 and p["picked"] == 0


def test_the_plan_takes_the_forced_tile_or_the_automatic_choice_only(D):
    rc, _, err = plan(D, PLAIN, tile=22)
    assert rc == 1 and "tile_cfg 22" in err


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def made():
    cache = {}

    def get(c):
        if c.id not in cache:
            inp = P.make(c)
            cache[c.id] = (inp, P.reference(c, inp))
        return cache[c.id]
    return get


def test_the_table_is_small_where_it_claims_to_be():
    assert {(c.M // P.BM, c.N // P.BN) for c in P.SMALL} == {(1, 8), (2, 4), (2, 5), (3, 5), (5, 3), (9, 1)}
    assert all(c.act != G.ACT_GELU or c.M * c.N <= 2816 * 3072 for c in P.CASES)      # (the float64 erf)
    assert max(c.M * c.N for c in P.CASES) == 11008 * 3072


@pytest.mark.parametrize("case", P.SMALL, ids=[c.id for c in P.SMALL])
def test_the_emulation_stays_inside_every_bound(case, made):
    inp, refs = made(case)
    for order in (0, 1):
        got = P.emulate_pp(case, inp, order)
        r = P.check(case, inp, got, refs)
        print(f"{case.id}: order {order}: worst error / bound of the restatement {max(r.values()):.3g}")
        assert max(r.values()) <= 1.0, (case.id, order, r)
        if P.is_bit_exact(case):
            assert {k: v for k, v in r.items() if k != "ostats"} == {k: 0.0 for k in r if k != "ostats"} and P.unequal(case, got, refs) == 0, (case.id, r)


@pytest.mark.parametrize("lc", P.LIVE_CASES, ids=[lc.id for lc in P.LIVE_CASES])
def test_the_live_emulation_stays_inside_every_bound(lc, made):
    inp = P.make_live(lc, made(lc.case)[0])
    refs = P.live_refs(lc, inp)
    got = P.emulate_pp(lc.case, inp, 0, live_rows=lc.m_live)
    r = P.check_live(lc, inp, got, 256, refs)
    assert max(r.values()) <= 1.0, (lc.id, r)
    assert not P.is_bit_exact(lc.case) or P.unequal_live(lc, got, refs) == 0
    if lc.panel_end < lc.case.M:      # a kernel that ignores the count is noticed: it overwrites sentinels
        bad = P.emulate_pp(lc.case, inp, 0)
        assert max(P.check_live(lc, inp, bad, 256, refs).values()) == math.inf, lc.id


KILLERS = {
    "second_tile_stored_at_first_tiles_coordinates": lambda c: True,
    "statistics_of_the_next_tile_in_the_epilogue": lambda c: P.mode_of(c) in ("fold", "rln"),
    "partial_beyond_count_not_zeroed": lambda c: P.mode_of(c) in ("fold", "rln") and c.parts < 24,
    "ragged_row_group_walked_as_full": lambda c: (c.M // P.BM) % P.PP_ROWS != 0,
    "residual_rows_read_with_ldo": lambda c: c.res == "bf16" and c.ldrb != c.ldo,
    "out_stats_rows_strided_by_the_tiles_partials": lambda c: c.out_stats and c.N > 128,
    "missing_bias_read_as_present": lambda c: not c.bias,
}


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_each_mutant_leaves_a_bound(mutant, made):
    killed = []
    if mutant == "dead_rows_of_the_live_panel_enter_the_guard":
        for lc in P.LIVE_CASES:
            if "guard" not in made(lc.case)[0] or lc.live % P.BM == 0:
                continue
            inp = P.make_live(lc, made(lc.case)[0])
            refs = P.live_refs(lc, inp)
            assert max(P.check_live(lc, inp, P.emulate_pp(lc.case, inp, 0, live_rows=lc.m_live), 256, refs).values()) <= 1.0
            r = P.check_live(lc, inp, P.emulate_pp(lc.case, inp, 0, mutant, live_rows=lc.m_live), 256, refs)
            if r["guard"] >= G.MUTANT_FACTOR:
                killed.append((lc.id, r["guard"]))
    else:
        for c in P.SMALL:
            if not KILLERS[mutant](c):
                continue
            inp, refs = made(c)
            worst = max(P.check(c, inp, P.emulate_pp(c, inp, 0, mutant), refs).values())
            if worst == math.inf if P.is_bit_exact(c) else worst >= G.MUTANT_FACTOR:
                killed.append((c.id, worst))
    print(f"{mutant}: leaves its bound on {len(killed)} cases: " + ", ".join(f"{i} ({w:.3g})" for i, w in killed[:4]))
    assert killed, mutant


def test_operands_are_poisoned_and_outputs_guarded(made):
    c = next(c for c in P.SMALL if P.mode_of(c) == "rln" and c.lda > c.K)
    inp, _ = made(c)
    for k, cols in (("A", c.K), ("W", c.K), ("resb", c.N)):
        b = G.bf16_f32(inp[k])
        assert np.isnan(b[:, cols:]).all() and np.isnan(b[-G.POST:]).all() and not np.isnan(b[:-G.POST, :cols]).any(), k
    assert np.isnan(inp["r_stats"][c.M:]).all() and np.isnan(inp["bias"][c.N:]).all() and np.isnan(inp["gamma"][c.N:]).all()
    assert (inp["ob"] == G.SENT_BF16).all() and inp["ob"].shape == (G.PRE + c.M + G.POST, c.ldo) and (inp["ostats"] == G.SENT_F32).all()
    assert len({c.lda, c.ldw, c.ldo, c.ldrb}) == 4
