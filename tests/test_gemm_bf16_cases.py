"""CPU: the case table of tests/test_gpu_gemm_bf16.py (tests/gemm_bf16_cases.py) reaches what it claims, and its bounds can tell a
wrong kernel from a rounded one.

The tile, m_tiles, n_tiles, xcd_cols and the statistics partial count of every case are read from the library's own host-side
argument checks and choice (ufnd_diag_gemm_bf16_plan: the product entries' checks, auto_cfg, xcd_cols_for, stat_parts_for; no launch,
no GPU), and the coverage list is asserted from those values and the tile table (bm, bn, ring depths) -- not from the case names.  A
retuned auto_cfg that moves a dgrad case off its tile fails here, and so does a tile added to the library without cases.

Which case kills which mutant: G.KILLS."""
import math

import numpy as np
import pytest

from tests import gemm_bf16_cases as G

FWD = ("gemm", "ex", "ln")


@pytest.fixture(scope="module")
def D():
    from tools import _diaglib
    _diaglib.diag()
    return _diaglib


def plan_args(c: G.Case, **over):
    """keyword arguments of _diaglib.gemm_bf16_plan for a case: made-up 16-B aligned addresses for the operands that are present"""
    from ultrafnd_git_amd import _lib as L
    a = 0x100000

    def addr(i, present=True):
        return a * (i + 1) if present else None
    kw = dict(A=addr(0), W=addr(1), bias=addr(2, c.bias), residual=addr(3, c.res in ("f32", "inplace")), aux=addr(4, c.act >= G.ACT_GELU_BWD),
              out_bf16=addr(5, c.outs != "f32"), out_f32=addr(3 if c.res == "inplace" else 6, c.outs != "bf16"), M=c.M, N=c.N, K=c.K, lda=c.lda,
              ldw=c.ldw, ldr=c.ldr, ldaux=c.ldaux, ldo=c.ldo, ldf=c.ldf, act=c.act, tile=c.tile)
    lnkw = None
    if c.entry == "ln":
        fold, rln = c.ln == "fold", c.ln == "rln"
        lnkw = dict(a_stats=addr(7, fold), colsum=addr(8, fold), r_stats=addr(9, rln), r_gamma=addr(10, rln), r_beta=addr(11, rln),
                    out_stats=addr(12, c.out_stats), a_parts=c.parts if fold else 0, r_parts=c.parts if rln else 0, a_eps=G.EPS, r_eps=G.EPS,
                    width=c.K if fold else c.N, tile_cfg=c.tile, residual_bf16=addr(13, c.res == "bf16"), ldrb=c.ldrb, guard=addr(14, c.guard != "no"))
    ln_over = over.pop("ln", {})
    kw.update(over)
    if lnkw is not None:
        lnkw.update(ln_over)
        kw["ln"] = L.GemmLn(**lnkw)
    return kw


def plan(D, c: G.Case, **over):
    return D.gemm_bf16_plan(c.entry, **plan_args(c, **over))


@pytest.fixture(scope="module")
def plans(D):
    out = {}
    for c in G.CASES:
        rc, p, err = plan(D, c)
        if c.refuse:
            assert rc == 1 and c.refuse in err, (c.id, rc, err)
        else:
            assert rc == 0, (c.id, err)
            out[c.id] = p
    return out


@pytest.fixture(scope="module")
def tiles(D):
    """the product tiles of the library: id -> plan fields (bm, bn, sta, stb, ln_aware, bwd)"""
    out, t = {}, 0
    while True:
        rc, p, _ = D.gemm_bf16_plan("tile", tile=t)
        if rc != 0:
            break
        if p["prod"]:
            out[t] = p
        t += 1
    assert t >= 29
    return out


def test_the_tile_table_of_the_cases_is_the_librarys(D, tiles):
    import ctypes as C
    from ultrafnd_git_amd import _lib as L
    assert set(tiles) == set(G.TILES), "a product tile without cases (or cases of a tile that is gone)"
    for t, p in tiles.items():
        bm, bn, sta, stb, _ = G.TILES[t]
        assert (p["bm"], p["bn"], p["sta"], p["stb"]) == (bm, bn, sta, stb), t
        b, n, ln = C.c_int(), C.c_int(), C.c_int()
        assert L.lib().ufnd_gemm_bf16_tile_info(t, C.byref(b), C.byref(n), C.byref(ln)) == 1 and (b.value, n.value, ln.value) == (bm, bn, p["ln_aware"])
    assert {t for t, p in tiles.items() if p["ln_aware"]} == set(G.LN_TILES)
    assert {t for t, p in tiles.items() if p["bwd"]} == set(G.BWD_TILES)
    for t in range(L.lib().ufnd_gemm_bf16_tile_count()):
        assert bool(L.lib().ufnd_gemm_bf16_tile_info(t, None, None, None)) == (t in tiles), t


def test_every_case_runs_on_the_tile_and_grid_it_names(plans):
    for c in G.CASES:
        if c.refuse:
            continue
        p = plans[c.id]
        assert p["tile"] == c.want, (c.id, p)
        assert (p["m_tiles"], p["n_tiles"]) == G.grid_of(c.want, c.M, c.N), (c.id, p)
        assert p["stat_parts"] == (c.N // 32 if c.out_stats else 0), (c.id, p)
        assert c.out_stats == (c.out_stats and G.has_stats_epilogue(c.want, c.N))
        assert 64 <= c.K <= 320 and c.K % 64 == 0 and p["n_tiles"] <= 4 or c.entry == "dgrad", c.id
        if c.M > 1100:
            assert c.entry == "dgrad" and c.K == 64 and c.want in (15, 22), c.id


def coverage_gaps(cases, plans, tiles):
    """the entries of the issue's coverage list that the table does not reach"""
    gaps = []
    live = [c for c in cases if not c.refuse]
    P = {c.id: plans[c.id] for c in live}

    def any_(pred, cs=live):
        return any(pred(c, P[c.id]) for c in cs)
    for t, tp in tiles.items():
        bm, bn, sta, stb = tp["bm"], tp["bn"], tp["sta"], tp["stb"]
        want_nk = {d + o for d in (sta, stb) for o in (-1, 0, 1) if d + o >= 1}
        fwd = [c for c in live if c.entry in FWD and P[c.id]["tile"] == t]
        modes = [("plain kernel", lambda c: c.entry in ("gemm", "ex"))]
        if tp["ln_aware"]:
            modes += [(f"ln {m}", lambda c, m=m: c.entry == "ln" and c.ln == m) for m in ("fold", "rln", "plain")]
        for name, sel in modes:
            have = {c.K // 64 for c in fwd if sel(c)}
            if not want_nk <= have:
                gaps.append(f"tile {t} {name}: nk {sorted(want_nk - have)} against ring depths {sta} / {stb}")
        for M in (1, bm - 1, bm + 1):
            if not any(c.M == M for c in fwd):
                gaps.append(f"tile {t}: M = {M}")
        if not any_(lambda c, p: p["xcd_cols"] == 2 and p["m_tiles"] >= 4 and p["n_tiles"] % 2 == 0, fwd):
            gaps.append(f"tile {t}: xcd_cols == 2")
        odd_ok = bn % 64 == 0          # an odd column-tile count needs n bn % 64 == 0 with n odd
        if not any_(lambda c, p: (p["m_tiles"] * p["n_tiles"]) % 8 != 0 and ((p["m_tiles"] * p["n_tiles"]) % 2 == 1 or not odd_ok), fwd):
            gaps.append(f"tile {t}: remap remainder")
        if odd_ok and not any_(lambda c, p: p["m_tiles"] >= 4 and p["n_tiles"] % 2 == 1, fwd):
            gaps.append(f"tile {t}: four row tiles, odd n_tiles")
        if tp["ln_aware"]:
            for res in ("f32", "bf16"):
                for parts in G.R_PARTS:
                    for os_ in (False, True):
                        def hit(c):
                            return (c.entry == "ln" and c.want == t and c.ln == "rln" and c.res == res and c.parts == parts and c.out_stats == os_
                                    and c.N % bn == 0 and c.family == "rounded")
                        got = [c for c in cases if hit(c)]
                        # (a refusal stands in only where the tile has no statistics epilogue; test_every_case.. / plans check its words)
                        if not got or any(c.refuse and G.has_stats_epilogue(t, c.N) for c in got):
                            gaps.append(f"tile {t}: rln residual {res} r_parts {parts} out_stats {os_}")
    plain = [c for c in live if c.entry in ("gemm", "ex") and c.ln == "none"]
    for bias in (True, False):
        for act in (0, 1, 2):
            for res in ("f32", "none"):
                for outs in ("bf16", "f32", "both"):
                    if not any((c.bias, c.act, c.res, c.outs) == (bias, act, res, outs) for c in plain):
                        gaps.append(f"plain epilogue: bias {bias} act {act} residual {res} outputs {outs}")
    if not any(c.res == "inplace" and c.ldr == c.ldf for c in plain):
        gaps.append("plain epilogue: in place")
    for entry, names in (("gemm", ("lda", "ldw", "ldr", "ldo", "ldf")), ("ex", ("lda", "ldw", "ldr", "ldo", "ldf")),
                         ("ln", ("lda", "ldw", "ldr", "ldo", "ldf")), ("ln", ("lda", "ldw", "ldrb", "ldo", "ldf")),
                         ("dgrad", ("lda", "ldw", "ldr", "ldo", "ldf")), ("dgrad", ("lda", "ldw", "ldaux", "ldo", "ldf"))):
        def strided(c):
            tight = dict(lda=c.K, ldw=c.K, ldr=c.N, ldo=c.N, ldf=c.N, ldrb=c.N, ldaux=c.N)
            used = dict(ldr=c.res == "f32", ldrb=c.res == "bf16", ldaux=c.act >= G.ACT_GELU_BWD, ldo=c.outs != "f32", ldf=c.outs != "bf16")
            vals = [getattr(c, n) for n in names]
            return c.entry == entry and len(set(vals)) == len(vals) and all(getattr(c, n) > tight[n] and used.get(n, True) for n in names)
        if not any(strided(c) for c in live):
            gaps.append(f"strides: {entry} {names}")
    fold = [c for c in live if c.entry == "ln" and c.ln == "fold" and c.family == "rounded"]
    for act in (0, 1, 2):
        for parts in G.A_PARTS:
            for guard in ("no", "yes"):
                if not any((c.act, c.parts, c.guard) == (act, parts, guard) for c in fold):
                    gaps.append(f"fold: act {act} a_parts {parts} guard {guard}")
    if not any(c.guard == "nan" for c in fold):
        gaps.append("fold: NaN statistic")
    if not any(c.entry == "ln" and c.ln == "plain" and c.res == "bf16" and c.out_stats and c.family == "rounded" for c in live):
        gaps.append("ln: neither statistics, residual_bf16 + out_stats")
    dg = [c for c in live if c.entry == "dgrad"]
    for t, tp in tiles.items():
        if tp["bwd"] and not any(P[c.id]["tile"] == t and c.M % tp["bm"] != 0 for c in dg):
            gaps.append(f"dgrad: tile {t} with ragged M")
    for act, res in ((0, "none"), (0, "f32"), (G.ACT_GELU_BWD, "none"), (G.ACT_QUICK_GELU_BWD, "none")):
        for outs in ("bf16", "f32", "both"):
            if not any((c.act, c.res, c.outs) == (act, res, outs) and (act == 0 or c.ldaux > c.N) for c in dg):
                gaps.append(f"dgrad: act {act} residual {res} outputs {outs}")
    for fam in ("exact", "rounded"):
        for name, sel in (("plain", lambda c: c.entry in ("gemm", "ex")), ("fold", lambda c: c.ln == "fold"), ("rln", lambda c: c.ln == "rln"),
                          ("ln plain", lambda c: c.ln == "plain"), ("dgrad", lambda c: c.entry == "dgrad")):
            if not any(sel(c) and c.family == fam for c in live):
                gaps.append(f"family {fam}: {name}")
    return gaps


def test_the_table_covers_the_list(plans, tiles):
    assert coverage_gaps(G.CASES, plans, tiles) == []


@pytest.mark.parametrize("drop,word", [
    (lambda c: c.want == 22 and c.ln == "fold" and c.K == 64, "tile 22 ln fold"),
    (lambda c: c.want == 20 and c.entry in ("gemm", "ex") and c.K == 320, "tile 20 plain kernel"),
    (lambda c: c.want == 2 and c.M == 3 * 256 + 5 and c.N == 256, "tile 2: xcd_cols"),
    (lambda c: c.want == 17 and c.M == 2 * 128 + 37, "tile 17: remap remainder"),
    (lambda c: c.want == 8 and c.M == 255, "tile 8: M = 255"),
    (lambda c: c.want == 28 and c.ln == "rln" and c.parts == 12 and c.res == "bf16" and not c.out_stats and c.family == "rounded", "tile 28: rln"),
    (lambda c: c.entry == "dgrad" and c.want == 15, "dgrad: tile 15"),
    (lambda c: c.res == "inplace", "in place"),
    (lambda c: c.guard == "nan", "NaN statistic"),
    (lambda c: c.entry == "gemm" and not c.bias and c.act == 2 and c.res == "none" and c.outs == "f32", "plain epilogue"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_coverage_notices_a_removed_entry(plans, tiles, drop, word):
    kept = [c for c in G.CASES if not drop(c)]
    assert len(kept) < len(G.CASES)
    gaps = coverage_gaps(kept, plans, tiles)
    assert gaps and any(word in g for g in gaps), gaps


def test_a_moved_dgrad_choice_is_noticed(plans, tiles):
    """what a retuned auto_cfg would do: the tile-22 dgrad cases planned on tile 17 instead"""
    moved = {k: (dict(v, tile=17) if G.BY_ID[k].entry == "dgrad" and v["tile"] == 22 else v) for k, v in plans.items()}
    assert any("dgrad: tile 22" in g for g in coverage_gaps(G.CASES, moved, tiles))


# ---------------------------------------------------------------------------------------------------------------------
def _base(entry):
    return next(c for c in G.CASES if c.entry == entry and not c.refuse and (entry != "ln" or c.ln == "rln") and c.res == "f32" and c.outs == "both")


REFUSALS = [
    # (entry, overrides, ln overrides, words of the refusal)
    ("ex", dict(K=96), {}, "K%64==0"),
    ("ex", dict(tile=17, N=256), {}, "needs N % 192 == 0"),
    ("ex", dict(tile=3), {}, "not part of this library"),
    ("ex", dict(lda=64), {}, "A/W strides"),
    ("ex", dict(ldw=132), {}, "A/W strides"),
    ("ex", dict(ldr=126), {}, "residual alignment"),
    ("ex", dict(ldr=130), {}, "residual alignment"),
    ("ex", dict(ldo=132), {}, "out_bf16 alignment"),
    ("ex", dict(ldf=64), {}, "out_f32 alignment"),
    ("ex", dict(A=0x100008), {}, "16-B aligned"),
    ("ex", dict(act=3), {}, "act=3"),
    ("gemm", dict(M=0), {}, "M=0"),
    ("ln", dict(K=100), {}, "K%64==0"),
    ("ln", dict(), dict(a_stats=0x900000, colsum=0x900100, a_parts=4), "mutually exclusive"),
    ("ln", dict(), dict(residual_bf16=0x900000, ldrb=1024), "residual (fp32) and residual_bf16"),
    ("ln", dict(residual=None), dict(residual_bf16=0x900000, ldrb=8), "residual_bf16 alignment"),
    ("ln", dict(act=1), {}, "only fused together with a folded LayerNorm"),
    ("ln", dict(), dict(r_parts=3), "r_parts=3"),
    ("ln", dict(), dict(r_parts=26), "r_parts=26"),
    ("ln", dict(), dict(r_parts=0), "r_parts=0"),
    ("ln", dict(), dict(width=0), "width"),
    ("ln", dict(), dict(r_gamma=None), "r_stats needs residual"),
    ("ln", dict(), dict(tile_cfg=64), "persistent form"),
    ("dgrad", dict(K=32), {}, "K%64==0"),
    ("dgrad", dict(act=1), {}, "act=1"),
    ("dgrad", dict(act=G.ACT_GELU_BWD), {}, "aux (the pre-activations) goes with an activation backward"),
    ("dgrad", dict(aux=0x900000), {}, "aux (the pre-activations) goes with an activation backward"),
    ("dgrad", dict(act=G.ACT_GELU_BWD, aux=0x900000, ldaux=1024), {}, "no residual beside it"),
    ("dgrad", dict(act=G.ACT_QUICK_GELU_BWD, aux=0x900000, ldaux=8, residual=None), {}, "aux alignment"),
    ("dgrad", dict(lda=60), {}, "operand strides"),
]


@pytest.mark.parametrize("entry,over,ln_over,words", REFUSALS, ids=[f"{e}-{w[:24].replace(' ', '_')}-{i}" for i, (e, _, _, w) in enumerate(REFUSALS)])
def test_the_launchers_refuse(D, entry, over, ln_over, words):
    c = _base(entry)
    rc, _, err = plan(D, c)
    assert rc == 0, err
    rc, _, err = plan(D, c, ln=ln_over, **over) if entry == "ln" else plan(D, c, **over)
    assert rc == 1 and words in err, (rc, err)


def test_fold_refusals(D):
    c = next(c for c in G.CASES if c.ln == "fold" and not c.refuse)
    for ln_over, over, words in ((dict(a_parts=5), {}, "a_parts=5"), (dict(a_parts=0), {}, "a_parts=0"), (dict(a_parts=26), {}, "a_parts=26"),
                                 (dict(out_stats=0x900000), {}, "takes no residual and writes no out_stats"),
                                 ({}, dict(residual=0x900000), "takes no residual"), (dict(colsum=None), {}, "colsum / a_stats alignment")):
        rc, _, err = plan(D, c, ln=ln_over, **over)
        assert rc == 1 and words in err, (ln_over, over, rc, err)


# ---------------------------------------------------------------------------------------------------------------------
def test_the_measured_activation_errors_are_what_the_formulas_promise():
    """ceilings from the formulas, not from the measurement: GELU: 1.5e-7 |erf error| x |x| / 2 (<= 3e-7 where the tail is non-zero, |x| < 6)
    plus four roundings of a result below 4 (4 x 2^-24 x 4); quick-GELU: three roundings of a result up to ACT_RANGE; the gradients: values
    below 1.13 (+ 1.702 |x| (1 - s) s), six to eight roundings"""
    m = G.measure_act_errors()
    assert m[G.ACT_GELU] <= 3e-7 + 16 * G.U + 5e-8 and m[G.ACT_QUICK_GELU] <= 3 * G.U * G.ACT_RANGE
    assert m[G.ACT_GELU_BWD] <= 8 * G.U * 1.13 and m[G.ACT_QUICK_GELU_BWD] <= 16 * G.U * 1.13


@pytest.fixture(scope="module")
def made():
    cache = {}

    def get(c):
        if c.id not in cache:
            inp = G.make(c)
            cache[c.id] = (inp, G.reference(c, inp))
        return cache[c.id]
    return get


SMALL = [c for c in G.CASES if not c.refuse and c.M <= 1100]
LARGE = [c for c in G.CASES if not c.refuse and c.M > 1100]


@pytest.mark.parametrize("entry", ("gemm", "ex", "ln", "dgrad"))
def test_a_float32_restatement_stays_inside_every_bound(entry, made):
    worst = (0.0, "-")
    for c in SMALL:
        if c.entry != entry:
            continue
        inp, refs = made(c)
        for order in (0, 1):
            got = G.emulate(c, inp, order)
            r = G.check(c, inp, got, refs)
            m = max(r.values())
            assert m <= 1.0, (c.id, order, r)
            if G.is_bit_exact(c):
                assert {k: v for k, v in r.items() if k != "ostats"} == {k: 0.0 for k in r if k != "ostats"} and G.unequal(c, got, refs) == 0, (c.id, r)
            worst = max(worst, (m, c.id))
    print(f"{entry}: worst error / bound of the restatement {worst[0]:.3g} at {worst[1]}")


@pytest.mark.parametrize("case", LARGE, ids=[c.id for c in LARGE])
def test_the_large_dgrad_cases_are_exact_in_the_restatement(case):
    inp = G.make(case)
    refs = G.reference(case, inp)
    got = G.emulate(case, inp, 1)
    assert max(G.check(case, inp, got, refs).values()) == 0.0 and G.unequal(case, got, refs) == 0


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_each_mutant_leaves_a_bound(mutant, made):
    c = G.BY_ID[G.KILLS[mutant]]
    inp, refs = made(c)
    good = max(G.check(c, inp, G.emulate(c, inp, 0), refs).values())
    r = G.check(c, inp, G.emulate(c, inp, 0, mutant), refs)
    worst = max(r.values())
    print(f"{mutant}: error / bound {worst:.3g} at {c.id} (unmutated {good:.3g})")
    assert good <= 1.0
    assert worst == math.inf if G.is_bit_exact(c) else worst >= G.MUTANT_FACTOR, (mutant, c.id, r)


def test_operand_rows_are_distinguishable_and_poisoned():
    c = G.BY_ID[G.KILLS["two_tiles_swapped"]]
    inp = G.make(c)
    assert np.unique(inp["bias"][:c.N]).size == c.N
    for k, cols in (("A", c.K), ("W", c.K)):
        b = G.bf16_f32(inp[k])
        assert np.isnan(b[:, cols:]).all() and np.isnan(b[-G.POST:]).all() and not np.isnan(b[:-G.POST, :cols]).any()
    assert np.isnan(inp["res"][:, c.N:]).all() and np.isnan(inp["res"][c.M:]).all() and np.isnan(inp["bias"][c.N:]).all()
    for k in ("of", "ob"):
        assert (inp[k][:G.PRE] == (G.SENT_F32 if k == "of" else G.SENT_BF16)).all() and inp[k].shape[0] == G.PRE + c.M + G.POST
