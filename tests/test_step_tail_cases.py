"""CPU checks of tests/step_tail_cases.py: the suite of tests/test_gpu_step_tail.py can see what it claims to see.

  * the table reaches every grid class of the launchers (block counts, strides and sweeps recomputed from their formulas), every
    hyper-parameter set, every cross-entropy batch size, label set, entry and logit set;
  * the float32 restatement of every op stays inside the op's bound on every case and is bit-equal where the bound is 0;
  * every mutant breaks a bit-equality or leaves a bound by MUTANT_FACTOR on at least one case (the mutants of the cases above
    1M floats run only on their designated catchers, S.DESIGNATED: that is what keeps this file's run time near that of
    tests/test_frozen_ops_cases.py);
  * every size class is needed by a named mutant (S.CLASS_NEEDED_BY);
  * the C entries refuse bad arguments before any launch, with their name in the message.
Inputs and references are computed once per (op, case) and shared; the large ones are not kept."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import step_tail_cases as S

OPS = sorted(S.OPS)


def _make(op, i):
    return S.OPS[op].make(S.OPS[op].cases[i])


@functools.lru_cache(maxsize=None)
def _small(op, i):
    inp = _make(op, i)
    return inp, S.OPS[op].reference(S.OPS[op].cases[i], inp)


def _inp_ref(op, i):
    if S.is_large(op, S.OPS[op].cases[i]):
        inp = _make(op, i)
        return inp, S.OPS[op].reference(S.OPS[op].cases[i], inp)
    return _small(op, i)


def ratios(op, mutant=None, cases=None, stop_at=math.inf):
    worst, where = 0.0, None
    for i, case in enumerate(S.OPS[op].cases):
        if cases is not None and case not in cases:
            continue
        inp, refs = _inp_ref(op, i)
        r = max(S.check(op, case, inp, S.OPS[op].restate(case, inp, mutant), refs).values())
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
    if op in S.EXACT_OPS:
        assert worst == 0.0 or op == "adamw_zero_grad", (op, worst)      # (bc1 / bc2_sqrt of adamw_zero_grad carry one rounding)


@pytest.mark.parametrize("op,mutant", [(op, m) for op in OPS for m in S.OPS[op].mutants])
def test_mutant_is_caught(op, mutant):
    best, where = ratios(op, mutant, cases=S.designated_cases(op, mutant), stop_at=S.MUTANT_FACTOR)
    print(f"{op} / {mutant}: best error / bound {best:.3g} at {where}")
    assert best >= S.MUTANT_FACTOR, (op, mutant, best, where)


def test_required_mutants_are_present():
    have = {m for op in S.OPS.values() for m in op.mutants}
    need = {"last_float4_skipped", "pair_second_skipped", "tail_sweep_dropped_at_cap", "element_updated_twice", "finalize_first_256_partials",
            "norm_without_grad_scale", "update_with_abs_grad_scale", "clip_without_1e-6", "bias_corrections_at_t_minus_1",
            "beta1_in_second_correction", "eps_inside_sqrt", "weight_decay_folded_into_gradient", "step_advanced_twice", "micro_not_reset",
            "accumulate_adds_on_overwrite", "ce_mean_over_B", "smoothing_eps_not_halved", "smoothing_missing_from_d_logits",
            "row_max_not_subtracted"}
    assert need <= have, need - have
    for (op, m), sizes in S.DESIGNATED.items():
        assert m in S.OPS[op].mutants and set(sizes) <= {c[0] for c in S.OPS[op].cases}, (op, m)


def test_table_reaches_every_grid_class():
    H = S.HALF_CAP
    census = {c[0] for c in S.OPS["step_census"].cases}
    assert census == set(S.ALL_SIZES) and set(S.ALL_SIZES) == {n for cl in S.SIZE_CLASSES.values() for n in cl}
    assert S.ONE_BLOCK == (1, 63, 64, 65, 255, 256, 257)
    for n4 in S.ONE_BLOCK:
        assert S.adamw_grid(n4)[0] == 1 and S.norm_grid(n4) == (1, 256, 1 if n4 <= 256 else 2)
    assert S.pair_and_tail(256) == (0, 256) and S.pair_and_tail(257) == (2, 255)            # exactly one pair: elements 0 and 256
    assert [S.adamw_grid(n)[0] for n in (511, 512, 513)] == [1, 1, 2]
    assert S.pair_and_tail(512) == (512, 0) and S.pair_and_tail(513) == (2, 511)            # every element in a pair; the first pair of a two-block grid
    assert [S.norm_grid(n)[0] for n in (1023, 1024, 1025)] == [1, 1, 2]
    assert [S.norm_grid(n)[0] for n in S.FINALIZE] == [255, 256, 257, 1023] == list(S.FINALIZE_BLOCKS)
    assert S.CAPS == (2 * H, 2 * H + 1, 3 * H - 1, 3 * H + 1, 4 * H + 5) and H == 524_288
    for n4 in S.CAPS:
        assert S.adamw_grid(n4)[:2] == (S.ADAMW_CAP, H) and S.norm_grid(n4)[0] == S.NORM_CAP
    assert (2 * H + S.ADAMW_PER_BLOCK - 1) // S.ADAMW_PER_BLOCK == S.ADAMW_CAP and (2 * H + 1023) // 1024 == S.NORM_CAP      # the caps exactly, unclamped
    assert S.pair_and_tail(2 * H) == (2 * H, 0) and S.adamw_grid(2 * H)[2] == 2
    assert S.pair_and_tail(2 * H + 1) == (2 * H, 1) and S.adamw_grid(2 * H + 1)[2] == 3     # one element in a third sweep
    assert S.pair_and_tail(3 * H - 1) == (2 * H, H - 1) and S.pair_and_tail(3 * H + 1) == (2 * H + 2, H - 1)
    assert S.pair_and_tail(4 * H + 5) == (4 * H, 5) and S.adamw_grid(4 * H + 5)[2] == 5
    assert max(4 * n for n in S.ALL_SIZES) <= 8_400_000
    # the census premise: no block of the norm can leave the integers of fp32
    for n4 in S.ALL_SIZES:
        assert S.norm_grid(n4)[2] * 256 * 4 * 14 * 14 < 2 ** 24, n4
    large = [(op, c) for op in OPS for c in S.OPS[op].cases if S.is_large(op, c)]
    assert 9 <= len(large) <= 11, len(large)
    assert all(4 * c[0] <= S.LARGE_FLOATS for op in ("accumulate", "adamw_zero_grad", "adamw_rounded") for c in S.OPS[op].cases)
    # a sub-range call: pointers 4 k floats into a larger buffer, k odd (16-B aligned and no more)
    assert {lo for _, lo in S.OPS["step_census"].cases} == {64, 148} and 148 % 4 == 0 and (148 // 4) % 2 == 1
    assert any(lo == 148 for n4, lo in S.OPS["step_census"].cases if n4 in S.CAPS)
    # accumulate: both arms, with and without the state, at every small size
    acc = S.OPS["accumulate"].cases
    assert {c[0] for c in acc} == set(S.SMALL_SIZES) and {c[1:] for c in acc} == {("bits", True), ("bits", False), ("add", True), ("add", False)}
    src = S.OPS["accumulate"].make((257, "bits", True))["src"]
    assert np.isnan(src).sum() >= 3 and np.signbit(src[src == 0]).any() and np.isnan(src[-1])
    # selection: the first, the last, both sides of a sweep edge and of a block edge, a block behind the finalize's first 256
    pos = S.select_positions(2 * H + 1)
    blocks, stride, sweeps = S.norm_grid(2 * H + 1)
    assert sweeps == 5 and {0, 4 * (2 * H + 1) - 1, 4 * stride - 1, 4 * stride, 4 * 4 * stride, 1023, 1024, 4 * 256 * 256} <= set(pos)
    assert S.select_positions(1) == [0, 3]
    # the norm: three scales, three grad scales, every clip kind
    nc = S.OPS["norm_clip"].cases
    assert {c[1] for c in nc} == set(S.NORM_SCALES) and {c[2] for c in nc} == set(S.NORM_GS) and {c[4] for c in nc} == set(S.CLIP_KINDS) | {None}
    assert {S.norm_grid(c[0])[2] for c in nc} >= {1, 3, 4} and max(S.norm_grid(c[0])[0] for c in nc) > 1
    # AdamW: every hyper-parameter set at every t; the eps elements; cancelling moments
    aw = S.OPS["adamw_rounded"].cases
    assert {(c[1], c[2]) for c in aw} == {(h, t) for h in S.ADAMW_HPS for t in S.ADAMW_T} and {c[0] for c in aw} == set(S.ADAMW_SIZES)
    assert {S.adamw_grid(n)[0] for n in S.ADAMW_SIZES} == {1, 2, 5}
    for i, case in enumerate(aw):
        inp, refs = _small("adamw_rounded", i)
        idx = inp["eps_idx"]
        assert len(idx) == S.EPS_ELEMENTS and not inp["g"][idx].any() and not inp["v"][idx].any() and inp["m"][idx].all()
        hp = inp["hp"]
        coef = refs["clip_coef"][0][0]
        assert (coef < 1.0) == (case[1] in ("trainer_clip_active", "negative_grad_scale")), (case, coef)
        assert (np.sign(inp["m"]) * np.sign(inp["g"] * hp.gs) < 0).mean() > 0.3       # a b1 and (1 - b1) g of opposite signs
    assert S.COUNTER_RUNS == ((0, 3), (99_999, 1))
    # cross-entropy
    ce = S.OPS["cross_entropy"].cases
    assert {c[0] for c in ce} == set(S.CE_B) == {1, 2, 63, 64, 65, 255, 256, 257, 513, 1000}
    for B in S.CE_B:
        mine = [c for c in ce if c[0] == B]
        assert {c[1] for c in mine} == set(S.CE_LABELS) and {c[2] for c in mine} == set(S.CE_ENTRIES) and {c[3] for c in mine} == set(S.CE_LOGITS), B
        assert {(c[1], c[2]) for c in mine} == {(l, e) for l in S.CE_LABELS for e in S.CE_ENTRIES}, B
    for e in S.CE_ENTRIES:
        assert {c[3] for c in ce if c[2] == e} == set(S.CE_LOGITS), e
    grid, shifted = ({c[:3] for c in ce if c[3] == k} for k in ("grid", "grid_shifted"))
    assert grid == shifted and len(grid) >= 2 * len(S.CE_B)      # EVERY grid case is repeated with 1024 added: same batch, labels, entry
    for e in S.CE_ENTRIES:
        assert any(c[2] == e for c in grid), e
    a, b = (S.OPS["cross_entropy"].make((257, "mixed", None, k))["logits"] for k in ("grid", "grid_shifted"))
    assert np.array_equal(a.astype(np.float64) + S.CE_SHIFT, b.astype(np.float64)) and np.abs(a).max() <= 8
    assert np.array_equal(a * 1024, np.round(a * 1024))
    mix = S.OPS["cross_entropy"].make((257, "mixed", None, "one_of_each"))["logits"].astype(np.float64)
    gaps = np.abs(mix[:, 0] - mix[:, 1])
    assert (gaps == 0).any() and (np.abs(gaps - 20) < 1e-4).any() and (np.abs(gaps - 90) < 1e-4).any() and (np.abs(gaps - 120) < 1e-4).any()
    assert np.exp(-90.0) < S.TINY and np.exp(-120.0) < 2.0 ** -149      # the loser's exponential underflows: below the normals, below the denormals


def test_every_size_class_is_needed_by_a_mutant():
    assert set(S.CLASS_NEEDED_BY) == set(S.SIZE_CLASSES)
    for cl, (op, mutant, only) in S.CLASS_NEEDED_BY.items():
        mine = [c for c in S.OPS[op].cases if c[0] in S.SIZE_CLASSES[cl]]
        small = [c for c in mine if not S.is_large(op, c)] or mine
        best, where = ratios(op, mutant, cases=small, stop_at=S.MUTANT_FACTOR)
        assert best >= S.MUTANT_FACTOR, (cl, mutant, best)
        if only:      # nothing outside the class sees it (the small and medium cases: the other large ones are other classes' business)
            others = [c for c in S.OPS[op].cases if c[0] not in S.SIZE_CLASSES[cl] and not S.is_large(op, c)]
            worst, where = ratios(op, mutant, cases=others)
            assert worst <= 1.0, (cl, mutant, worst, where)
    # the mutants that only some sizes of a class can see
    see = lambda m, n4: ratios("step_census", m, cases=[c for c in S.OPS["step_census"].cases if c[0] == n4])[0] >= S.MUTANT_FACTOR
    assert not see("pair_second_skipped", 256) and see("pair_second_skipped", 257) and see("pair_second_skipped", 513)
    assert not see("finalize_reads_one_partial", 1024) and see("finalize_reads_one_partial", 1025)
    assert not see("finalize_first_256_partials", S.FINALIZE[1]) and see("finalize_first_256_partials", S.FINALIZE[2])
    assert not see("tail_sweep_dropped_at_cap", 1025)


# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    import torch  # noqa: F401  (its HIP runtime must be resident before the library's is resolved)
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def _refused(rc, lib, word):
    msg = lib.ufnd_last_error()
    assert rc == 1 and msg and word in msg, (rc, msg, word)


def test_entries_refuse_bad_arguments_before_any_launch():
    """No GPU: every call returns UFND_ERR_INVALID before a launch (the pointers are never dereferenced on the host)."""
    lib = _lib()
    A, Bq, Cq, Dq, PT, ST, LB = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000      # 16-B aligned, far apart
    n = 64
    # ufnd_grad_accumulate(dst, src, n, overwrite, state, stream)
    for args in ((None, Bq, n, 1, ST, None), (A, None, n, 1, ST, None), (A, Bq, 0, 1, ST, None), (A, Bq, n + 2, 1, ST, None), (A + 4, Bq, n, 1, ST, None),
                 (A, Bq + 4, n, 0, None, None), (A, A + 16, n, 1, None, None), (A + 16, A, n, 0, None, None), (A, A, n, 0, None, None)):
        _refused(lib.ufnd_grad_accumulate(*args), lib, b"grad_accumulate:")
    _refused(lib.ufnd_grad_accumulate(A, A + 16, n, 1, None, None), lib, b"overlap")
    _refused(lib.ufnd_grad_accumulate(A + 16, A, n, 1, None, None), lib, b"overlap")
    # ufnd_grad_norm(grad, n, partials, state, stream)
    for args in ((None, n, PT, ST, None), (A, n, None, ST, None), (A, n, PT, None, None), (A, 0, PT, ST, None), (A, n + 1, PT, ST, None), (A + 4, n, PT, ST, None)):
        _refused(lib.ufnd_grad_norm(*args), lib, b"grad_norm:")
    # ufnd_adamw_step(param, grad, exp_avg, exp_avg_sq, n, state, stream)
    good = [A, Bq, Cq, Dq]
    for k in range(4):
        for bad in (None, good[k] + 4):
            ptrs = list(good)
            ptrs[k] = bad
            _refused(lib.ufnd_adamw_step(*ptrs, n, ST, None), lib, b"adamw_step:")
            _refused(lib.ufnd_clip_adamw_step(*ptrs, n, PT, ST, None), lib, b"clip_adamw_step:")
    for nn in (0, n + 3):
        _refused(lib.ufnd_adamw_step(*good, nn, ST, None), lib, b"adamw_step:")
        _refused(lib.ufnd_clip_adamw_step(*good, nn, PT, ST, None), lib, b"clip_adamw_step:")
    _refused(lib.ufnd_adamw_step(*good, n, None, None), lib, b"adamw_step:")
    _refused(lib.ufnd_clip_adamw_step(*good, n, None, ST, None), lib, b"clip_adamw_step:")
    _refused(lib.ufnd_clip_adamw_step(*good, n, PT, None, None), lib, b"clip_adamw_step:")
    # the state holds uint64 counters: 4 bytes off its alignment is refused by every entry that takes one
    _refused(lib.ufnd_grad_accumulate(A, Bq, n, 1, ST + 4, None), lib, b"grad_accumulate:")
    _refused(lib.ufnd_grad_norm(A, n, PT, ST + 4, None), lib, b"grad_norm:")
    _refused(lib.ufnd_grad_norm(A, n, PT + 2, ST, None), lib, b"grad_norm:")
    _refused(lib.ufnd_adamw_step(*good, n, ST + 4, None), lib, b"adamw_step:")
    _refused(lib.ufnd_clip_adamw_step(*good, n, PT, ST + 4, None), lib, b"clip_adamw_step:")
    _refused(lib.ufnd_clip_adamw_step(*good, n, PT + 2, ST, None), lib, b"clip_adamw_step:")
    # ufnd_step_advance(state, stream)
    _refused(lib.ufnd_step_advance(None, None), lib, b"step_advance:")
    _refused(lib.ufnd_step_advance(ST + 4, None), lib, b"step_advance:")
    # ufnd_softmax_ce(logits, labels, B, loss_rows, d_logits, state, stream): the labels are int64 and the state holds a uint64
    for args in ((None, LB, 4, None, None, ST, None), (A, None, 4, None, None, ST, None), (A, LB, 4, None, None, None, None), (A, LB, 0, None, None, ST, None),
                 (A, LB, -1, None, None, ST, None), (A, LB + 4, 4, None, None, ST, None), (A, LB, 4, None, None, ST + 4, None)):
        _refused(lib.ufnd_softmax_ce(*args), lib, b"softmax_ce:")
    F = ctypes.c_float
    for args in ((None, LB, 4, None, None, ST, None), (A, None, 4, None, None, ST, None), (A, LB, 4, None, None, None, None), (A, LB, 0, None, None, ST, None),
                 (A, LB + 4, 4, None, None, ST, None), (A, LB, 4, None, None, ST + 4, None)):
        _refused(lib.ufnd_softmax_ce_weighted(*args[:3], F(1), F(1), F(0), *args[3:]), lib, b"softmax_ce_weighted:")
    for w0, w1, eps in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 1.0, 0.0), (1.0, -0.5, 0.0), (1.0, 1.0, -0.01), (1.0, 1.0, 1.0), (1.0, 1.0, 1.5),
                        (float("nan"), 1.0, 0.0), (1.0, 1.0, float("nan"))):
        _refused(lib.ufnd_softmax_ce_weighted(A, LB, 4, F(w0), F(w1), F(eps), None, None, ST, None), lib, b"softmax_ce_weighted:")
