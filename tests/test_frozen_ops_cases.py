"""CPU checks of tests/frozen_ops_cases.py: the suite of tests/test_gpu_frozen_ops.py can see what it claims to see.

  * the float32 restatement of every op stays inside the op's bound on every case (the bound is not too tight for a correct fp32
    implementation that sums in another order);
  * every mutant -- a deliberately wrong restatement -- leaves the bound by MUTANT_FACTOR on at least one case of its op;
  * the table reaches all four NI instances of every NI_LAUNCH op, both arms of ufnd_attention_bf16 and ufnd_vit_patchify, odd grid
    sizes and every edge the cases are named for;
  * the probes' premises hold: the selection margin, the exactness of the census inputs.
Restatement outputs are computed once per (op, case) and shared."""
import functools
import math

import numpy as np
import pytest

from tests import frozen_ops_cases as F

OPS = sorted(F.OPS)


@functools.lru_cache(maxsize=None)
def _inputs(op, i):
    return F.OPS[op].make(F.OPS[op].cases[i])


@functools.lru_cache(maxsize=None)
def _refs(op, i):
    return F.OPS[op].reference(F.OPS[op].cases[i], _inputs(op, i))


def ratios(op, mutant=None, stop_at=math.inf):
    """(worst error / bound, its case) of the restatement (or a mutant of it) over the op's cases"""
    worst, where = 0.0, None
    for i, case in enumerate(F.OPS[op].cases):
        inp = _inputs(op, i)
        with np.errstate(invalid="ignore"):
            r = max(F.check(op, case, inp, F.OPS[op].restate(case, inp, mutant), _refs(op, i)).values())
        if r > worst:
            worst, where = r, case
        if worst >= stop_at:
            break
    return worst, where


@pytest.mark.parametrize("op", OPS)
def test_fp32_restatement_stays_inside_the_bound(op):
    worst, where = ratios(op)
    print(f"{op}: restatement worst error / bound {worst:.3g} at {where}")
    assert worst <= 1.0, (op, worst, where)


@pytest.mark.parametrize("op,mutant", [(op, m) for op in OPS for m in F.OPS[op].mutants])
def test_mutant_leaves_the_bound(op, mutant):
    best, where = ratios(op, mutant, stop_at=F.MUTANT_FACTOR)      # (tools/frozen_ops_errors.py reports the best over all cases)
    print(f"{op} / {mutant}: best error / bound {best:.3g} at {where}")
    assert best >= F.MUTANT_FACTOR, (op, mutant, best, where)


def test_required_mutants_are_present():
    need = {"layernorm": {"one_pass_variance", "divide_by_h_minus_1", "beta_before_gamma"},
            "bert_embed": {"position_row_div_L", "no_clamp"},
            "vit_assemble": {"position_shifted_by_one", "class_row_only_for_sample_0", "stats_before_layernorm"},
            "vit_patchify": {"ky_kx_swapped"},
            "masked_meanpool_l2": {"divide_by_L", "last_live_token_dropped"},
            "l2norm_frames": {"no_per_frame_normalisation", "no_final_normalisation"},
            "field_mean_l2": {"divide_by_Mx"}}
    for probe in ("attention_select", "attention_census", "attention_general"):
        need[probe] = {"last_key_of_a_block_dropped", "mask_shifted_by_one", "all_masked_row_is_zeros"}
    for op, ms in need.items():
        assert ms <= set(F.OPS[op].mutants), op


def test_bf16_helpers():
    x = F.cast_specials()
    b = F.bf16_bits(x)
    f = lambda u32: np.array([u32], dtype=np.uint32).view(np.float32)
    assert F.bf16_bits(f(0x3F808000))[0] == 0x3F80 and F.bf16_bits(f(0x3F818000))[0] == 0x3F82      # ties go to even
    assert F.bf16_bits(f(0x3F808001))[0] == 0x3F81 and F.bf16_bits(f(0x3F807FFF))[0] == 0x3F80
    assert F.bf16_bits(f(0x7F7F8000))[0] == 0x7F80 and F.bf16_bits(f(0x80000000))[0] == 0x8000      # overflow to inf; -0 stays
    assert np.isnan(F.bf16_f32(b)[np.isnan(x)]).all() and not np.isnan(F.bf16_f32(b)[~np.isnan(x)]).any()
    assert F.bf16_ulp(1.0) == 2.0 ** -7 and F.bf16_ulp(0.75) == 2.0 ** -8 and F.bf16_ulp(0.0) == 0.0
    # half an ulp of bf16 reaches 2^-8 of the value, which is why BF is 2^-8
    assert abs(float(F.bf16_round(f(0x3F808000))[0]) - (1 + 2.0 ** -8)) == 2.0 ** -8 and F.BF == 2.0 ** -8
    assert F.worst_ratio(np.array([np.nan, 1.0]), np.array([np.nan, 1.0]), np.zeros(2)) == 0.0
    assert F.worst_ratio(np.array([1.0]), np.array([np.nan]), np.ones(1)) == math.inf
    assert F.worst_ratio(np.array([np.inf, 1.0]), np.array([np.inf, 1.5]), np.array([0.0, 1.0])) == 0.5


def test_table_reaches_every_instance_and_edge():
    ln = F.OPS["layernorm"].cases
    for H in F.LN_H:
        mine = [c for c in ln if c[0] == H]
        assert {c[1] for c in mine} == set(F.LN_M)
        assert {c[2] - H for c in mine} == {0, 4} and {c[3] for c in mine} == set(F.LN_OUT) and {c[4] for c in mine} == set(F.LN_EPS), H
        kinds = {F.ROW_KINDS[(c[5] + r) % 3] for c in mine for r in range(c[1])}
        assert kinds == set(F.ROW_KINDS)
    assert {c[0] // 256 for c in ln} == set(F.NI_VALUES)
    for op in ("bert_embed", "vit_assemble"):
        assert {c[0] // 256 for c in F.OPS[op].cases} == set(F.NI_VALUES), op
    assert {(c[3], c[4]) for c in F.OPS["bert_embed"].cases} == set(F.EMB_FORMS)
    assert {c[3] for c in F.OPS["vit_assemble"].cases} == set(F.ASM_VARIANTS)
    for op, rows in (("layernorm", lambda c: c[1]), ("bert_embed", lambda c: c[1] * c[2]), ("vit_assemble", lambda c: c[1] * (c[2] + 1))):
        m = {rows(c) for c in F.OPS[op].cases}
        assert 1 in m or 2 in m, op                                     # a single workgroup with idle waves
        assert any(r % 4 for r in m) and any(r > 4 for r in m), op      # a ragged last workgroup, more than one workgroup
    ids = F.OPS["bert_embed"].make((256, 3, 5, "ln", "f32"))["ids"]
    assert {-1, F.EMB_VOCAB, 2 ** 40} <= set(ids.tolist())
    # patchify: both dispatch arms
    arms = {(patch, image // patch) == F.PATCHIFY_FAST for image, patch, _ in F.OPS["vit_patchify"].cases}
    assert arms == {True, False}
    assert len({patch for image, patch, _ in F.OPS["vit_patchify"].cases if (patch, image // patch) != F.PATCHIFY_FAST}) >= 3
    # attention: both arms, the boundary on both sides, odd grids, grids that are no multiple of 8, every 64-key block edge
    grid = F.ATTN_GRID
    Ls = {L for _, L, _ in grid}
    assert {F.ATTN_SHORT_L, F.ATTN_SHORT_L + 1} <= Ls and min(Ls) == 1 and max(Ls) > 1024
    assert {63, 64, 65, 127, 129, 193, 513} <= Ls
    sizes = [F.attn_grid_size(*g) for g in grid]
    assert sum(s % 2 for s in sizes) >= 5 and sum(s % 8 != 0 for s in sizes) >= 8 and any(s > 8 and s % 8 for s in sizes)
    for n in sizes:          # the block-id remapping of the kernel is a bijection at every grid size in the table
        q, r = n >> 3, n & 7
        ids = sorted((x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (i >> 3) for i in range(n) for x in [i & 7])
        assert ids == list(range(n)), n
    for B, L, heads in grid:
        for kind in F.ATTN_MASKS[1:]:
            m = F.attn_mask(kind, B, L)
            assert m.shape == (B, L) and m[0].any()
            assert B == 1 or not m[1].any()             # one all-masked sample where B > 1
    assert not F.attn_mask("hole", 1, 193)[0, 64:128].any() and F.attn_mask("hole", 1, 193)[0, 63] and F.attn_mask("hole", 1, 193)[0, 128]
    assert not F.attn_mask("left", 1, 129)[0, :64].any() and F.attn_mask("single", 1, 129)[0].sum() == 1
    # pooled ops
    assert {L for _, L in F.OPS["masked_meanpool_l2"].cases} == {1, 31, 32, 33, 77}
    inp = F.OPS["masked_meanpool_l2"].make((256, 33))
    assert np.isnan(inp["hidden"][inp["mask"] == 0]).all() and not np.isnan(inp["hidden"][inp["mask"] != 0]).any()
    assert not inp["mask"][3].any() and inp["mask"][2].sum() == 1 and inp["mask"][2, -1] == 1 and inp["mask"][1, 1] == 0 and inp["mask"][1, 3] == 1
    e = F.OPS["l2norm_frames"].make((2, 8, 1024))["e"].astype(np.float64)
    nrm = np.sqrt((e * e).sum(-1))
    assert nrm[0, -1] == 0 and nrm[nrm > 0].min() <= 1.1e-3 and nrm.max() >= 0.9e3
    fld = F.OPS["field_mean_l2"].make((4, 12, 768))
    assert sorted(fld["valid"].sum(-1).tolist()) == [0, 1, 6, 12] and np.isnan(fld["parts"][fld["valid"] == 0]).all()
    # elementwise ops
    assert F.CAST_GRID_CAP + 3 in F.OPS["cast_bf16"].cases and {1, 3, 4, 5, 1023} <= set(F.OPS["cast_bf16"].cases)
    big = F.OPS["cast_bf16"].make(F.CAST_GRID_CAP + 3)["x"]
    assert np.isnan(big[-3:]).any() or np.isinf(big[-3:]).any() or (big[-3:] == 0).any()      # specials in the scalar tail
    assert {n for _, n in F.OPS["act_bf16"].cases} == {65280, F.ACT_GRID_CAP + 8}
    assert len(F.GATHER_ITEMS) == F.GATHER_MAX_ITEMS and {8, 8 * 129, 3072} <= {b for b, _ in F.GATHER_ITEMS}
    assert len({r for _, r in F.GATHER_ITEMS}) > 3 and min(F.GATHER_IDX) < 0 and max(F.GATHER_IDX) >= min(r for _, r in F.GATHER_ITEMS)
    assert len(set(F.GATHER_IDX)) < len(F.GATHER_IDX)


def test_selection_probe_margin():
    """Every selected score exceeds every other live score of its row by at least 40 nats, so every other probability is below
    exp(-40) = 4.3e-18 and the selected value comes out bit for bit."""
    worst = math.inf
    for i, case in enumerate(F.OPS["attention_select"].cases):
        m = F.select_margin(case, _inputs("attention_select", i))
        assert m >= F.SELECT_MARGIN, (case, m)
        worst = min(worst, m)
    print(f"selection probe: least margin {worst:.1f} nats")
    inp = _inputs("attention_select", F.OPS["attention_select"].cases.index((3, 65, 5, "hole")))
    v = F.bf16_f32(inp["qkv"]).reshape(3 * 65, 3, 5 * 64)[:, 2]
    assert (np.abs(v) >= 0.5).all() and (np.abs(v) <= 8).all()          # bf16-exact by construction: they ARE bf16 values
    pi, mask = inp["pi"], inp["mask"]
    for h in range(5):
        live = np.flatnonzero(mask[0])
        assert set(pi[0, h].tolist()) == set(live.tolist())             # a permutation of the live keys, reused cyclically


def test_census_probe_inputs_are_exact():
    for i, case in enumerate(F.OPS["attention_census"].cases):
        B, L, heads, _ = case
        qkv = _inputs("attention_census", i)["qkv"].reshape(B * L, 3, heads * 64)
        assert not qkv[:, 0].any()                                        # Q = +0 exactly: every score is 0, every p is 1
        assert set(np.unique(qkv[:, 2]).tolist()) <= {0x0000, 0x3F80}     # V holds 0 and 1 only
        v = qkv[:, 2].reshape(B, L, heads, 64)
        assert ((v[0, :, 0] == 0x3F80) == (np.arange(L)[:, None] % 64 == np.arange(64)[None, :])).all()
        assert L / 64 <= 18                                               # a channel counts at most 18 keys: one key is >= 1/18 of it
