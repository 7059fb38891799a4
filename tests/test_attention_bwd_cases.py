"""CPU checks of tests/attention_bwd_cases.py: the suite of tests/test_gpu_attention_bwd.py can see what it claims to see.

  * the case table covers every length, head count, grid size, mask kind, dropout length and family the cases are named for;
  * the float32 restatement stays inside the bound on every case -- on an exact case it reproduces the reference bit for bit, in
    NumPy's summation order and in the reversed one (the evidence that those sums are exact in any order);
  * every mutant -- a deliberately wrong backward -- breaks a bit-equality or leaves the bound by MUTANT_FACTOR on at least one case;
  * the probes' premises hold: the selection margin, power-of-two live counts, bf16-exact operands, and that the reference's repeated
    roundings are the identity without dropout.
References and inputs are computed once per case and shared."""
import functools
import math

import numpy as np
import pytest

from tests import attention_bwd_cases as A

N = len(A.CASES)


@functools.lru_cache(maxsize=None)
def _inputs(i):
    return A.make(A.CASES[i])


@functools.lru_cache(maxsize=None)
def _refs(i):
    return A.reference(A.CASES[i], _inputs(i))


def test_case_table_covers_the_list():
    C = A.CASES
    exact = [c for c in C if A.is_exact(c)]
    rounded = [c for c in C if c.family == "rounded"]
    assert all(c.B * c.heads <= 3 * 17 and c.L <= 1100 for c in C)
    # lengths: each in an exact and in a rounded case with B, heads <= 2; one L = 1100 (nob = 9)
    for L in A.L_ALL:
        assert any(c.L == L and c.B <= 2 and c.heads <= 2 for c in exact), L
        assert any(c.L == L and c.B <= 2 and c.heads <= 2 for c in rounded), L
    assert any(c.L == A.L_LONG for c in exact) and any(c.L == A.L_LONG for c in rounded) and -(-A.L_LONG // A.OB) == 9
    # heads at L = 65, exact through dQ (K free) and dK (Q free); beyond the delta kernel's pass also rounded
    for h in A.HEADS_AT_65:
        assert any(c.L == 65 and c.heads == h for c in exact), h
    for h in (9, 17):
        assert {c.family for c in C if c.L == 65 and c.heads == h} >= {"census_q0", "census_k0", "rounded"}, h
    # grids: the remap's remainder 0, 1 and 7, and a grid below 8 (quotient 0)
    sizes = {A.grid_size(c) for c in C}
    assert set(A.GRIDS) <= sizes, sorted(sizes)
    assert {0, 1, 7} <= {g & 7 for g in A.GRIDS} and any(g < 8 for g in A.GRIDS)
    for n in sizes:          # the kernel's block-id remap is a bijection at every grid size in the table
        q, r = n >> 3, n & 7
        ids = sorted((x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (i >> 3) for i in range(n) for x in [i & 7])
        assert ids == list(range(n)), n
    # B = 3 with a different mask per sample
    for c in C:
        if c.B == 3 and c.mask != "none":
            m = A.case_mask(c)
            assert len({m[b].tobytes() for b in range(3)}) == 3, c
    assert any(c.B == 3 and A.is_exact(c) for c in C) and any(c.B == 3 for c in rounded)
    # masks: every kind, in an exact and in a rounded case; the blocked kinds really mask their block between live keys
    for kind in A.MASK_KINDS:
        big = kind in ("block64", "own128")
        assert any(c.mask == kind and (not big or c.L > 2 * A.WB) for c in exact), kind
        assert any(c.mask == kind and (not big or c.L > 2 * A.WB) for c in rounded), kind
    m = A.mask_row("block64", 193, True)
    assert not m[64:128].any() and m[:64].any() and m[128:].any() and m.sum() == 128
    m = A.mask_row("own128", 320, False)
    assert not m[128:256].any() and m[:128].all() and m[256:].all()
    assert not A.mask_row("own128", 257, True)[128:256].any() and not A.mask_row("own128", 193, True)[:128].any()
    assert A.mask_row("last", 129, True).tolist() == [0] * 128 + [1] and A.mask_row("first", 129, True).sum() == 1
    h = A.mask_row("holes", 65, False)
    assert h[0] and not h[1] and h[2] and h[64] and not h[32:40].any()
    for c in C:
        if c.mask == "dead":
            m = A.case_mask(c)
            assert c.B >= 2 and not m[1].any() and m[0].any()
    dead = [c for c in C if c.mask == "dead"]
    assert any(A.is_exact(c) and c.p == 0 for c in dead) and any(c.L == 50 and not A.is_exact(c) for c in dead)
    assert any(c.p == 0.5 for c in dead) and any(c.p == 0.1 for c in dead)
    # masked queries carry a live dctx in every family: dctx has no zero row anywhere
    for fam in ("census_q0", "census_k0", "select", "rounded"):
        i = next(i for i, c in enumerate(C) if c.family == fam and c.mask not in ("none", "ones"))
        d = A.bf16_f32(_inputs(i)["dctx"]).reshape(C[i].B * C[i].L, C[i].heads, 64)
        assert (np.abs(d).sum(-1) > 0).all(), fam
    # dropout: 0.5 exact and 0.1 rounded at every listed length; L % 4 in 0 .. 3 among the exact ones
    for L in A.DROP_L:
        assert any(c.L == L and c.p == 0.5 and A.is_exact(c) for c in C), L
        assert any(c.L == L and c.p == 0.1 and c.family == "rounded" for c in C), L
    assert {c.L % 4 for c in C if c.p == 0.5 and A.is_exact(c)} == {0, 1, 2, 3}
    # selection: every kind of pi
    assert {c.variant for c in C if c.family == "select"} == set(A.SELECT_KINDS)
    # rounded: flat and peaked rows
    assert {c.variant for c in rounded} == {"flat", "peaked"}
    # the census's not-a-power-of-two live counts fall under the rounded bound
    assert any(c.family.startswith("census") and not A.is_exact(c) and c.p == 0 and c.mask != "dead" for c in C)
    assert set(A.MUTANTS) >= {"walked_tail_block_dropped", "walked_block_visited_twice", "clamped_rows_not_silenced", "key_mask_shifted_by_one",
                              "mask_of_sample_0_for_every_sample", "delta_of_head_h_plus_1", "delta_skipped_for_heads_ge_8",
                              "form2_half_tiles_exchanged", "owned_tiles_swapped", "scale_missing", "pass2_nibble_indexed_by_key", "lp4_is_L_shr_2"}


@pytest.mark.parametrize("i", range(N), ids=[A.case_id(c) for c in A.CASES])
def test_fp32_restatement_stays_inside_the_bound(i):
    c = A.CASES[i]
    res = A.check(c, A.restate(c, _inputs(i)), _refs(i))
    print(f"{A.case_id(c)}: " + ", ".join(f"{k} {r:.3g} ({n} outside)" for k, (r, n) in res.items()))
    for k, (r, n) in res.items():
        assert n == 0 and r <= 1.0, (c, k, r, n)


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutant_is_caught(mutant):
    hits, tried = [], 0
    for i, c in enumerate(A.CASES):
        if not A.mutant_applies(mutant, c) or c.L > 520:
            continue
        tried += 1
        with np.errstate(invalid="ignore"):
            res = A.check(c, A.restate(c, _inputs(i), mutant), _refs(i))
        if A.caught(c, res):
            hits.append((A.case_id(c), res["dqkv"]))
            if len(hits) >= 3:
                break
    print(f"{mutant}: caught by {hits} (of {tried} cases tried)")
    assert hits, mutant


@pytest.mark.parametrize("mutant", A.WALK_MUTANTS)
def test_walk_mutant_is_caught_where_the_walk_has_several_blocks(mutant):
    """At L <= 64 a dropped or doubled "block" is everything.  The concern is one lost, doubled or leaked row among hundreds: every exact
    case with more than one walked block (L = 65: the dropped tail block is ONE row of 65; L = 257: one of 257) must lose a bit-equality."""
    tried = []
    for i, c in enumerate(A.CASES):
        if not (A.is_exact(c) and A.WB < c.L <= 520 and A.mutant_applies(mutant, c)):
            continue
        with np.errstate(invalid="ignore"):
            res = A.check(c, A.restate(c, _inputs(i), mutant), _refs(i))
        tried.append((A.case_id(c), res["dqkv"]))
        assert A.caught(c, res) and res["dqkv"][1] > 0, (mutant, c, res)
    print(f"{mutant}: unequal dqkv elements per case {[(n, r[1]) for n, r in tried]}")
    lengths = {int(n.split("-")[2]) for n, _ in tried}
    assert {65, 129, 193, 257, 513} <= lengths, sorted(lengths)


def test_exact_probes_premises():
    worst = math.inf
    for i, c in enumerate(A.CASES):
        inp = _inputs(i)
        if c.family == "select":
            m = A.select_margin_log2(c, inp)
            assert m >= A.SELECT_MARGIN_LOG2, (c, m)
            worst = min(worst, m)
            x = A.bf16_f32(inp["qkv"]).reshape(c.B * c.L, 3, c.heads * 64)
            assert set(np.unique(np.abs(x[:, 0]))) == {16.0} and set(np.unique(np.abs(x[:, 1]))) == {4.0}
            for t in (x[:, 2], A.bf16_f32(inp["dctx"])):
                assert (t * 4 == np.round(t * 4)).all() and np.abs(t).max() < 4
            if c.variant == "many_to_one" and c.L >= 15:
                assert len(set(inp["pi"][0, 0].tolist())) < c.L          # several queries select one key
            if inp["mask"] is not None:
                for b in range(c.B):
                    assert inp["mask"][b][inp["pi"][b]].all()             # never a masked key
        elif A.is_exact(c):
            mask = inp["mask"]
            live = A.live_keys(c, mask)
            v = A.census_values(c, mask)
            x = A.bf16_f32(inp["qkv"]).reshape(c.B * c.L, 3, c.heads, 64)
            zero_part = 0 if c.family == "census_q0" else 1
            assert not inp["qkv"].reshape(c.B * c.L, 3, c.heads * 64)[:, zero_part].any()      # +0 exactly: every score is 0
            assert (x[:, 2] == v.reshape(-1)[:, None, None]).all()                             # V_j = v_j in every channel, bf16-exact
            for b in range(c.B):
                idx = np.flatnonzero(live[b]) if live[b].any() else np.arange(c.L)
                n = idx.size
                assert n & (n - 1) == 0 and v[b, idx].sum() % n == 0
                vbar = v[b, idx].sum() // n
                assert np.abs(v[b, idx] - vbar).max() < 256 and 1 <= v[b].min() and v[b].max() <= 242
            if c.p == 0:      # without dropout the roundings the reference repeats are the identity: it IS the plain definition
                plain = A.reference(c._replace(family="rounded"), inp)
                for k in ("ctx", "dqkv"):
                    assert np.array_equal(plain[k][0], _refs(i)[k][0]), (c, k)
    print(f"selection probes: least margin {worst:.1f} (base 2)")
    assert A.rne_bf16(np.array([1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8 - 2.0 ** -40])).tolist() == \
        [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6, -1 - 2.0 ** -7]              # ties to even; no double rounding through fp32
    assert A.judge(np.array([1.0, 2.0]), np.array([1.0, 2.0]), np.zeros(2)) == (0.0, 0)
    assert A.judge(np.array([1.0, np.nan]), np.array([1.0, 2.0]), np.ones(2))[1] == 1
    assert A.judge(np.array([1.0078125]), np.array([1.0]), np.zeros(1)) == (math.inf, 1)
    assert A.judge(np.array([1.0]), np.array([1.003]), np.zeros(1)) == (0.0, 0)                      # RNE(1.003) = 1
    r, n = A.judge(np.array([1.0078125]), np.array([1.003]), np.full(1, 0.002))                      # needs 0.00090625 of the 0.002
    assert n == 0 and abs(r - 0.453125) < 1e-9
    assert A.judge(np.array([-1.0078125]), np.array([-1.003]), np.full(1, 0.0005))[1] == 1
    assert A.judge(np.array([0.0, 0.0]), np.array([0.0, 1e-30]), np.zeros(2)) == (math.inf, 1)
    assert A.judge(np.array([3.0], dtype=np.float32), np.array([3.0 + 1e-9]), np.zeros(1), fp32=True) == (0.0, 0)


@pytest.mark.parametrize("i", [i for i, c in enumerate(A.CASES) if A.is_exact(c) and c.L <= 520], ids=lambda i: A.case_id(A.CASES[i]))
def test_exact_sums_do_not_depend_on_the_order(i):
    """The restatement with every sequence reversed (queries and keys: NumPy then adds in the opposite order) gives the same bits."""
    c = A.CASES[i]
    inp = _inputs(i)
    B, L, heads = c.B, c.L, c.heads
    flip = lambda a, w: a.reshape(B, L, w)[:, ::-1].reshape(B * L, w)
    rev = dict(inp, qkv=flip(inp["qkv"], 3 * heads * 64), dctx=flip(inp["dctx"], heads * 64),
               mask=None if inp["mask"] is None else inp["mask"][:, ::-1], dm=None if inp["dm"] is None else inp["dm"][:, :, ::-1, ::-1])
    a, b = A.restate(c, inp), A.restate(c, rev)
    assert np.array_equal(a["dqkv"], flip(b["dqkv"], 3 * heads * 64)) and np.array_equal(a["ctx"], flip(b["ctx"], heads * 64))
