"""CPU checks of tests/audio_ops_cases.py: the suite of tests/test_gpu_audio_ops.py can see what it claims to see.

  * the float32 restatement of every op stays inside the op's bound on every case (bit-equal where the bound is 0);
  * every mutant leaves the bound by MUTANT_FACTOR (or breaks an equality) on at least one case of its op;
  * the pivot-sensitive arithmetic -- fp32 sums about a chunk's FIRST value, m2 = q - s^2 / n -- leaves the bound of both statistics
    kernels by MUTANT_FACTOR on the clips whose 100-sigma click is a chunk's first value, is MUTANT_FACTOR x worse than the re-centred
    arithmetic on the 10- and 20-sigma ones (the figures are in that test's docstring), and stays inside on every other clip;
  * the table holds the lengths, shapes and data kinds it is meant to.
Restatement outputs are computed once per (op, case) and shared."""
import functools
import math

import numpy as np
import pytest

from tests import audio_ops_cases as A

OPS = sorted(A.OPS)


@functools.lru_cache(maxsize=None)
def _inputs(op, i):
    return A.OPS[op].make(A.OPS[op].cases[i])


@functools.lru_cache(maxsize=None)
def _refs(op, i):
    return A.OPS[op].reference(A.OPS[op].cases[i], _inputs(op, i))


def ratio(op, i, mutant=None) -> float:
    case = A.OPS[op].cases[i]
    with np.errstate(invalid="ignore"):
        return max(A.check(op, case, _inputs(op, i), A.OPS[op].restate(case, _inputs(op, i), mutant), _refs(op, i)).values())


@pytest.mark.parametrize("op", OPS)
def test_fp32_restatement_stays_inside_the_bound(op):
    rs = [(ratio(op, i), c) for i, c in enumerate(A.OPS[op].cases)]
    worst, where = max(rs, key=lambda t: t[0])
    print(f"{op}: restatement worst error / bound {worst:.3g} at {A.case_id(where)}")
    assert worst <= 1.0, (op, worst, where)
    if op in ("w2v2_frames", "w2v2_pos_pack", "w2v2_pos_add"):
        assert worst == 0.0


@pytest.mark.parametrize("op,mutant", [(op, m) for op in OPS for m in A.OPS[op].mutants if m != "pivot_sensitive"])
def test_mutant_leaves_the_bound(op, mutant):
    best, where = 0.0, None
    for i, c in enumerate(A.OPS[op].cases):
        r = ratio(op, i, mutant)
        if r > best:
            best, where = r, c
        if best >= A.MUTANT_FACTOR:
            break
    print(f"{op} / {mutant}: best error / bound {best:.3g} at {A.case_id(where)}")
    assert best >= A.MUTANT_FACTOR, (op, mutant, best, where)


@pytest.mark.parametrize("op", ("wave_normalize", "w2v2_conv0"))
def test_the_bound_sees_the_pivot_sensitive_arithmetic_and_only_there(op):
    """Sums about a chunk's first value, on every clip of the table.  Where the click IS a chunk's first value:
      100 sigma   error / bound 24.5 and 23.4 (ufnd_wave_normalize, click at sample 4096 / 0), 6.82 (ufnd_w2v2_conv0, frame 256): the
                  bound is left by MUTANT_FACTOR;
      20 sigma    ufnd_wave_normalize 3.71 and 1.54: the bound is left, by less than MUTANT_FACTOR;
      10 sigma    ufnd_w2v2_conv0 0.403: INSIDE the bound.  The bound charges every one of the d = 66 additions a full rounding, the
                  defect grows with (click / sigma)^2: at 10 sigma it is 12 x the re-centred arithmetic's error on the same clip and
                  still below the worst case a correct kernel is allowed.
    So the per-element bound proves the defect at 100 sigma; at 10 - 20 sigma what is asserted is that the pivot-sensitive error is
    MUTANT_FACTOR x the re-centred one on the same clip.  (The kernels before the re-centring measured these same ratios on the
    MI355X to three digits: profiles/audio_ops_errors.txt.)  On every other clip the two arithmetics stay inside the bound."""
    at_start = A.is_chunk_start_click if op == "wave_normalize" else A.is_chunk_start_frame_click
    left = 0
    for i, c in enumerate(A.OPS[op].cases):
        r, good = ratio(op, i, "pivot_sensitive"), ratio(op, i)
        print(f"{op} {A.case_id(c)}: pivot-sensitive error / bound {r:.3g} (re-centred {good:.3g})")
        assert good <= 1.0
        if not at_start(c[0]):
            assert r <= 1.0, (op, c, r)
        elif c[0].startswith("click100"):
            assert r >= A.MUTANT_FACTOR, (op, c, r)
            left += 1
        else:
            assert r >= A.MUTANT_FACTOR * good, (op, c, r, good)
    assert left == (2 if op == "wave_normalize" else 1)


def test_the_table_holds_what_it_is_meant_to():
    fr = A.OPS["w2v2_frames"]
    n = set(fr.make(("all", 1))["lengths"].tolist())
    assert set(range(400, 2101)) <= n and {16000, 41360, 41680, 480000, 2 ** 24 + 7} <= n
    assert {c[1] for c in fr.cases if c[0] == "all"} == {1, 2, 131} and ("30s", 1500) in fr.cases
    assert [A.hf_frames(k) for k in (400, 719, 720, 16000, 41360, 41680, 480000)] == [1, 1, 2, 49, 129, 130, 1499]
    assert A.OPS["w2v2_pos_pack"].cases == A.OPS["w2v2_pos_add"].cases == [(1, 1, (1,)), (3, 5, (1, 5, 3)), (2, 131, (130, 64))]
    pk = A.OPS["w2v2_pos_pack"].make((3, 5, (1, 5, 3)))
    assert (pk["x"][1] == A.NAN_BF16).all() and (pk["x"][5:10] != A.NAN_BF16).all() and (pk["x"][13:15] == A.NAN_BF16).all()
    ad = A.OPS["w2v2_pos_add"].make((3, 5, (1, 5, 3)))
    assert np.isnan(ad["x"][1:5]).all() and np.isnan(ad["conv"][:, 1:5 + 128]).all() and not np.isnan(ad["conv"][:, 0]).any()
    assert A.POSCONV_CASE == (4, 66, (1, 3, 64, 65))
    wv = A.OPS["wave_normalize"].cases
    assert {c[1][0] for c in wv if c[0] == "smooth" and len(c[1]) == 1} == {400, 4095, 4096, 4097, 8192, 8193, 12289}
    assert sum(len(c[1]) == 3 for c in wv) == 1 and {c[0] for c in wv} == {"smooth"} | set(A.WAVE_KINDS)
    assert 12289 % A.WCH == 1 and sum(A.is_chunk_start_click(k) for k in A.WAVE_KINDS) == 4
    w = A.OPS["wave_normalize"].make(("smooth", A.WAVE_BATCH))["wave"]
    assert all(np.isnan(w[b, k:]).all() and not np.isnan(w[b, :k]).any() for b, k in enumerate(A.WAVE_BATCH))
    x = A.wave_clip("click100_at_4096", A.WAVE_N).astype(np.float64)
    assert abs((x[4096] - np.delete(x, 4096).mean()) / np.delete(x, 4096).std() - 100) < 3
    c0 = A.OPS["w2v2_conv0"].cases
    assert {A.conv0_T1(c[1][0]) for c in c0 if c[0] == "smooth" and len(c[1]) == 1} == {79, 128, 255, 256, 257, 513}
    assert {c[2] for c in c0 if c[0] == "smooth"} == {0, 64} and {c[0] for c in c0} == {"smooth"} | set(A.CONV0_KINDS)
    assert A.conv0_S1((645,), 0) == 128 and A.conv0_S1((400,), 64) == 192 and A.conv0_T1(A.CONV0_N) > 257
    assert 5 * 256 <= 1287 < 5 * 256 + 10 and not 5 * 255 <= 1287 < 5 * 255 + 10 and not 5 * 256 <= 1292 < 5 * 256 + 10


def test_a_minus_zero_where_plus_zero_is_promised_is_unequal():
    case = (3, 5, (1, 5, 3))
    inp = A.OPS["w2v2_pos_add"].make(case)
    got = A.OPS["w2v2_pos_add"].restate(case, inp)
    assert max(A.check("w2v2_pos_add", case, inp, got).values()) == 0.0
    got["y"][1, 7] = np.float32(-0.0)
    assert max(A.check("w2v2_pos_add", case, inp, got).values()) == math.inf
