"""CPU checks of the raw-data recipe: focal loss, mixup, warm restarts.

  * tests/focal_cases.py: the table reaches every batch size, gap, offset, label set, labels_b set, lam and (alpha, gamma) the issue
    names; the float32 restatement of ufnd_softmax_focal stays inside the derived bound on every case; every named mistake leaves
    the bound by MUTANT_FACTOR on some case; the term-by-term bounds stay under the closed forms c(gap, gamma), c'(gap, gamma) of
    the module's docstring; the float32 1 - exp(-ce) of the reference's FocalLoss is as far off as the kernel's comment says;
  * the C entries refuse bad arguments before any launch, with the argument's name in the message;
  * optim.CosineAnnealingWarmRestarts equals torch's class over 40 epochs, to the last bit;
  * TrainConfig validates every new option and refuses the combinations by name; the defaults keep the fused two-call head path;
  * the mixup draw follows its seed, its probability and its mode; the CLI flags parse.
Inputs and references are computed once per case and shared."""
import ctypes
import functools
import math
import sys
import types

import numpy as np
import pytest

from tests import focal_cases as F

OP = F.OPS["focal"]


@functools.lru_cache(maxsize=None)
def _case(i):
    inp = OP.make(OP.cases[i])
    return inp, OP.reference(OP.cases[i], inp)


def ratios(mutant=None, stop_at=math.inf):
    worst, where = 0.0, None
    for i, case in enumerate(OP.cases):
        inp, refs = _case(i)
        r = max(F.check(case, inp, OP.restate(case, inp, mutant), refs).values())
        if r > worst:
            worst, where = r, case
        if worst >= stop_at:
            break
    return worst, where


def test_fp32_restatement_stays_inside_the_bound():
    worst, where = ratios()
    print(f"focal: restatement worst error / bound {worst:.3g} at {where}")
    assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_mutant_is_caught(mutant):
    best, where = ratios(mutant, stop_at=F.MUTANT_FACTOR)
    print(f"focal / {mutant}: best error / bound {best:.3g} at {where}")
    assert best >= F.MUTANT_FACTOR, (mutant, best, where)


def test_required_mutants_are_present():
    assert set(F.MUTANTS) == {"q_as_one_minus_pt", "pt_ce_term_missing", "gamma_minus_one_for_gamma", "lam_and_one_minus_lam_swapped",
                              "mean_over_2B", "labels_b_ignored", "alpha_missing_from_gradient"}


def test_table_reaches_what_the_issue_names():
    cases = OP.cases
    assert {c[0] for c in cases} == set(F.FOCAL_B) == {1, 2, 63, 64, 65, 255, 256, 257, 1000}
    assert set(F.GAPS) == {0.0, 1e-3, -1e-3, 1.0, -1.0, 12.0, -12.0, 30.0, -30.0, 100.0, -100.0} and set(F.OFFSETS) == {0.0, 1e3, -1e3}
    assert set(F.ALPHA_GAMMA) == {(1.0, 2.0), (0.25, 2.0), (1.0, 1.0), (1.0, 3.5), (1.0, 5.0), (1.0, 0.0)}
    assert set(F.LAMS) == {1.0, 0.0, 0.5, 1e-9, "beta"} and set(F.LABELS_B) == {None, "same", "reversed", "random"}
    for B in F.FOCAL_B:
        mine = [c for c in cases if c[0] == B]
        assert {(c[1], c[2]) for c in mine} == {(ag, l) for ag in F.ALPHA_GAMMA for l in F.LABELS}, B
        assert {c[3] for c in mine} == set(F.OFFSETS) and {c[4] for c in mine} == set(F.LABELS_B) and {c[5] for c in mine} == set(F.LAMS), B
    for ag in F.ALPHA_GAMMA:
        mine = [c for c in cases if c[1] == ag]
        assert {(c[4], c[5]) for c in mine if c[4] is not None} == {(lb, lam) for lb in F.LABELS_B[1:] for lam in F.LAMS}, ag
        assert any(c[4] is None for c in mine) and {c[3] for c in mine} == set(F.OFFSETS), ag
    # the rows of a batch walk through every gap; the logits hold the gap at every offset (to the offset's fp32 spacing)
    for i, c in enumerate(cases):
        inp, _ = _case(i)
        lg = inp["logits"].astype(np.float64)
        assert np.abs((lg[:, 0] - lg[:, 1]) - inp["gap"]).max() <= 2.0 ** -14, c
        if c[0] >= len(F.GAPS):
            assert set(inp["gap"]) == set(F.GAPS), c
        if c[4] is not None:
            assert inp["mix"].dtype == np.float32 and inp["labels_b"].shape == inp["labels_a"].shape
        if c[4] == "reversed":
            assert (inp["labels_a"] != inp["labels_b"]).any() or (c[0] <= 2 and c[2] == "mixed")
        if c[2] != "mixed":
            assert len(set(inp["labels_a"])) == 1
    # lam: the draws of Beta(0.2, 0.2) lie inside (0, 1); 1 - 1e-9 rounds to 1 in fp32 while 1e-9 does not vanish
    assert tuple(F.mix_of(1e-9)) == (np.float32(1e-9), np.float32(1.0)) and tuple(F.mix_of(1.0)) == (1.0, 0.0)
    beta = [float(_case(i)[0]["mix"][0]) for i, c in enumerate(cases) if c[5] == "beta" and c[4] is not None]
    assert len(beta) >= 20 and all(0.0 <= x <= 1.0 for x in beta) and len(set(beta)) > 10
    # the exact rows exist: labels on the winner at |gap| = 100, without and with mixup
    n_zero = {mixed: sum(int(F.zero_mask(_case(i)[0], c[1][1]).sum()) for i, c in enumerate(cases) if (c[4] is not None) == mixed) for mixed in (False, True)}
    assert n_zero[False] > 100 and n_zero[True] > 100, n_zero


def test_bounds_stay_under_the_closed_forms():
    """d_fl <= c(gap, gamma) u (|fl| + alpha q^gamma) and d_g <= c'(gap, gamma) u (|g| + alpha gamma q^gamma) on every unmixed row,
    to a floor of a few TINY"""
    worst_c = worst_cp = 0.0
    for i, case in enumerate(OP.cases):
        (alpha, gamma), inp = case[1], _case(i)[0]
        if gamma == 0:
            continue
        fl, d_fl, g, d_g, q = F.rows_ref_bound(inp["logits"], inp["labels_a"], alpha, gamma)
        c, cp = F.closed_form(np.abs(inp["gap"]), gamma)
        floor = 64 * F.TINY
        worst_c = max(worst_c, float(((d_fl - floor) / (c * F.U * (np.abs(fl) + alpha * q ** gamma) + 1e-300)).max()))
        worst_cp = max(worst_cp, float(((d_g - floor) / (cp[:, None] * F.U * (np.abs(g) + alpha * gamma * (q ** gamma)[:, None]) + 1e-300)).max()))
    print(f"term-by-term bound / closed form: loss {worst_c:.3g}, gradient {worst_cp:.3g}")
    assert worst_c <= 1.0 and worst_cp <= 1.0, (worst_c, worst_cp)


def test_one_minus_pt_in_fp32_is_off_by_a_fifth_at_gap_16():
    """why the kernel takes q from the softmax: the reference's float32 1 - exp(-ce) against the true q at a logit gap of 16"""
    import torch
    lg = torch.tensor([[16.0, 0.0]])
    ce = torch.nn.functional.cross_entropy(lg, torch.tensor([0]), reduction="none")
    q32 = float(1 - torch.exp(-ce))
    q = float(np.exp(-16.0) / (1 + np.exp(-16.0)))
    assert 0.05 <= abs(q32 - q) / q <= 0.5, (q32, q)


# ---------------------------------------------------------------------------------------------------------------------
def _lib():
    import torch  # noqa: F401  (its HIP runtime must be resident before the library's is resolved)
    from ultrafnd_git_amd import _lib as L
    return L


def _refused(rc, lib, word):
    msg = lib.ufnd_last_error()
    assert rc == 1 and msg and word in msg, (rc, msg, word)


def test_entries_refuse_bad_arguments_before_any_launch():
    """No GPU: every call returns UFND_ERR_INVALID before a launch (the pointers are never dereferenced on the host)."""
    L = _lib()
    lib, Fl = L.lib(), ctypes.c_float
    A, LA, LB, MX, ST = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    # ufnd_softmax_focal(logits, labels_a, labels_b, mix, B, alpha, gamma, loss_rows, d_logits, state, stream)
    ok = (Fl(1.0), Fl(2.0), None, None, ST, None)
    for head in ((None, LA, None, None, 4), (A, None, None, None, 4), (A, LA, None, None, 0), (A, LA, None, None, -3), (A, LA + 4, None, None, 4),
                 (A, LA, LB + 4, MX, 4), (A, LA, LB, MX + 2, 4)):
        _refused(lib.ufnd_softmax_focal(*head, *ok), lib, b"softmax_focal:")
    _refused(lib.ufnd_softmax_focal(A, LA, None, None, 4, Fl(1.0), Fl(2.0), None, None, None, None), lib, b"softmax_focal:")
    _refused(lib.ufnd_softmax_focal(A, LA, None, None, 4, Fl(1.0), Fl(2.0), None, None, ST + 4, None), lib, b"softmax_focal:")
    _refused(lib.ufnd_softmax_focal(A, LA, LB, None, 4, *ok), lib, b"labels_b and mix")
    _refused(lib.ufnd_softmax_focal(A, LA, None, MX, 4, *ok), lib, b"labels_b and mix")
    for alpha in (0.0, -1.0, float("inf"), float("nan")):
        _refused(lib.ufnd_softmax_focal(A, LA, None, None, 4, Fl(alpha), Fl(2.0), None, None, ST, None), lib, b"alpha=")
    for gamma in (-1.0, 0.5, 0.999, 5.001, 1e-6, float("inf"), float("nan")):
        _refused(lib.ufnd_softmax_focal(A, LA, None, None, 4, Fl(1.0), Fl(gamma), None, None, ST, None), lib, b"gamma=")
    # ufnd_gather_mix_rows(idx, perm, mix, B, items, n_items, n_groups, stream)
    IDX, PERM, SRC, DST, DSTB = 0x60000000, 0x70000000, 0x80000000, 0x90000000, 0xA0000000

    def items(*rows):
        arr = (L.MixItem * len(rows))()
        for it, (src, dst, dst_b, rb, n, kind, group) in zip(arr, rows):
            it.src, it.dst, it.dst_b, it.row_bytes, it.src_rows, it.kind, it.group = src, dst, dst_b, rb, n, kind, group
        return arr
    good = items((SRC, DST, None, 3072, 100, 0, 0))
    for args in ((None, PERM, MX, 4, good, 1, 1), (IDX, None, MX, 4, good, 1, 1), (IDX, PERM, None, 4, good, 1, 1), (IDX, PERM, MX, 0, good, 1, 1),
                 (IDX, PERM, MX, 4, None, 1, 1), (IDX, PERM, MX, 4, good, 0, 1), (IDX, PERM, MX, 4, good, 9, 1)):
        _refused(lib.ufnd_gather_mix_rows(*args, None), lib, b"gather_mix_rows:")
    for ng in (0, 9):
        _refused(lib.ufnd_gather_mix_rows(IDX, PERM, MX, 4, good, 1, ng, None), lib, b"n_groups=")
    _refused(lib.ufnd_gather_mix_rows(IDX + 4, PERM, MX, 4, good, 1, 1, None), lib, b"aligned")
    _refused(lib.ufnd_gather_mix_rows(IDX, PERM, MX + 2, 4, good, 1, 1, None), lib, b"aligned")
    for row, word in (((None, DST, None, 3072, 100, 0, 0), b"item 0"), ((SRC, None, None, 3072, 100, 0, 0), b"item 0"), ((SRC, DST, None, 4, 100, 0, 0), b"row_bytes=4"),
                      ((SRC, DST, None, 3076, 100, 0, 0), b"row_bytes=3076"), ((SRC, DST, None, 3072, 0, 0, 0), b"rows=0"), ((SRC, DST, None, 3072, 100, 2, 0), b"kind=2"),
                      ((SRC, DST, None, 3072, 100, 0, 1), b"group=1"), ((SRC, DST, None, 3072, 100, 0, -1), b"group=-1"), ((SRC, DST, None, 8, 100, 1, 0), b"dst_b"),
                      ((SRC + 4, DST, None, 3072, 100, 0, 0), b"aligned"), ((SRC, DST + 4, None, 3072, 100, 0, 0), b"aligned"),
                      ((SRC, DST, DSTB + 4, 8, 100, 1, 0), b"aligned")):
        _refused(lib.ufnd_gather_mix_rows(IDX, PERM, MX, 4, items(row), 1, 1, None), lib, word)
    assert ctypes.sizeof(L.MixItem) == 48


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_0,T_mult,eta_min", [(5, 2, 1e-6), (10, 2, 1e-6), (3, 1, 0.0)])
def test_warm_restarts_equal_torch_to_the_last_bit(T_0, T_mult, eta_min):
    import torch
    from ultrafnd_git_amd.optim import CosineAnnealingWarmRestarts
    lr = 2e-4
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    ref = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=T_0, T_mult=T_mult, eta_min=eta_min)

    class Stub:
        param_groups = [{"initial_lr": lr, "lr": lr}]

        def set_lr(self, v):
            self.param_groups[0]["lr"] = v
    mine = CosineAnnealingWarmRestarts(Stub(), T_0=T_0, T_mult=T_mult, eta_min=eta_min)
    assert mine.get_last_lr() == ref.get_last_lr() == [lr]
    seen = []
    for epoch in range(40):
        opt.step()
        ref.step()
        mine.step()
        assert mine.get_last_lr()[0] == ref.get_last_lr()[0], (epoch, mine.get_last_lr(), ref.get_last_lr())      # the same double
        assert (mine.T_cur, mine.T_i, mine.last_epoch) == (ref.T_cur, ref.T_i, ref.last_epoch), epoch
        seen.append(mine.get_last_lr()[0])
    assert seen.count(lr) >= (2 if T_mult == 2 else 10)      # the restarts happened
    for bad in (dict(T_0=0), dict(T_0=2.5), dict(T_0=3, T_mult=0), dict(T_0=True)):
        with pytest.raises(ValueError, match=next(iter(k for k in ("T_mult", "T_0") if k in bad))):
            CosineAnnealingWarmRestarts(Stub(), **bad)


def _cfg(**kw):
    from ultrafnd_git_amd.trainer import TrainConfig
    return TrainConfig(data_root="", ocr_phrase_pkl=None, **kw)


def test_train_config_validates_every_new_option_by_name():
    import dataclasses
    from ultrafnd_git_amd.trainer import TrainConfig
    c = _cfg()
    assert (c.criterion, c.focal_alpha, c.focal_gamma, c.mixup_alpha, c.mixup_prob, c.mixup_mode, c.warm_restarts) == ("ce", 1.0, 2.0, 0.0, 0.5, "shared", None)
    new = {"criterion", "focal_alpha", "focal_gamma", "mixup_alpha", "mixup_prob", "mixup_mode", "warm_restarts"}
    assert not new & {f.name for f in dataclasses.fields(TrainConfig)}      # init-only: the field list stays as pinned
    c = _cfg(criterion="focal", focal_alpha=0.25, focal_gamma=3.5, mixup_alpha=0.2, mixup_prob=1.0, mixup_mode="per_modality", warm_restarts=[5, 2, 1e-6])
    assert (c.criterion, c.focal_alpha, c.focal_gamma, c.mixup_alpha, c.mixup_prob, c.mixup_mode, c.warm_restarts) == \
        ("focal", 0.25, 3.5, 0.2, 1.0, "per_modality", (5, 2, 1e-6))
    bad = [("criterion", "bce"), ("criterion", None), ("focal_alpha", 0.0), ("focal_alpha", -1.0), ("focal_alpha", float("nan")), ("focal_alpha", "1"),
           ("focal_gamma", 0.5), ("focal_gamma", -1.0), ("focal_gamma", 5.5), ("focal_gamma", float("inf")), ("focal_gamma", True),
           ("mixup_alpha", -0.1), ("mixup_alpha", float("nan")), ("mixup_alpha", None), ("mixup_prob", -0.01), ("mixup_prob", 1.01), ("mixup_prob", "0.5"),
           ("mixup_mode", "each"), ("mixup_mode", None), ("warm_restarts", (5, 2)), ("warm_restarts", (0, 2, 1e-6)), ("warm_restarts", (5, 0, 1e-6)),
           ("warm_restarts", (5.5, 2, 1e-6)), ("warm_restarts", (5, 2, -1.0)), ("warm_restarts", 5)]
    for name, value in bad:
        with pytest.raises(ValueError, match=name):
            _cfg(**{name: value})


def test_refusals_name_their_arguments():
    from ultrafnd_git_amd.trainer import check_recipe
    for kw, names in ((dict(mixup_alpha=0.2, encode_inline=True), ("mixup_alpha", "encode_inline")),
                      (dict(mixup_alpha=0.2, train_encoders=True), ("mixup_alpha", "train_encoders")),
                      (dict(mixup_alpha=0.2, gnn_in_graph=True), ("mixup_alpha", "gnn_in_graph")),
                      (dict(criterion="focal", label_smoothing=0.1), ("focal", "label_smoothing")),
                      (dict(criterion="focal", class_weighting=True), ("focal", "class_weighting")),
                      (dict(warm_restarts=(5, 2, 1e-6), use_cosine=True), ("warm_restarts", "use_cosine"))):
        with pytest.raises(ValueError) as e:
            _cfg(**kw)
        assert all(n in str(e.value) for n in names), (kw, str(e.value))
    # a field set after construction is caught by the trainer's own check
    c = _cfg(mixup_alpha=0.2)
    c.gnn_in_graph = True
    with pytest.raises(ValueError, match="gnn_in_graph"):
        check_recipe(c)
    # what is allowed: focal with encode_inline, mixup with the CE criterion, warm restarts alone
    _cfg(criterion="focal", encode_inline=True), _cfg(mixup_alpha=0.2), _cfg(warm_restarts=(10, 2, 1e-6)), _cfg(mixup_alpha=0.0, encode_inline=True)


def _head(cfg, rank=0):
    import torch
    from ultrafnd_git_amd.head_step import HeadStep
    ns = types.SimpleNamespace
    return HeadStep(cfg, torch.device("cpu"), ns(), ns(eff_aux=2), ns(), ns(rank=rank, active=False))


def test_defaults_keep_the_fused_head_and_the_recipe_leaves_it():
    h = _head(_cfg())
    assert h.fused_entries is True and not h.focal and not h.mixup and h.mix_rng is None
    assert _head(_cfg(fused_head=False)).fused_entries is False
    assert _head(_cfg(criterion="focal")).fused_entries is False
    assert _head(_cfg(mixup_alpha=0.2)).fused_entries is False
    assert _head(_cfg(warm_restarts=(5, 2, 1e-6))).fused_entries is True
    assert _head(_cfg(mixup_alpha=0.2)).mix_groups == 1 and _head(_cfg(mixup_alpha=0.2, mixup_mode="per_modality")).mix_groups == 4


def test_the_draw_follows_seed_rank_probability_and_mode():
    B = 7
    a = [_head(_cfg(mixup_alpha=0.2, seed=5)).draw(B) for _ in range(1)]
    h1, h2, h3, h4 = (_head(_cfg(mixup_alpha=0.2, seed=s), rank=r) for s, r in ((5, 0), (5, 0), (6, 0), (5, 1)))
    d1, d2, d3, d4 = ([h.draw(B) for _ in range(40)] for h in (h1, h2, h3, h4))
    same = lambda x, y: all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(x, y))
    assert same(d1, d2) and not same(d1, d3) and not same(d1, d4) and same(a, d1[:1])
    ident = np.arange(B)
    mixed = 0
    for lams, perms in d1:
        assert lams.shape == (1,) and perms.shape == (1, B) and sorted(perms[0]) == list(ident) and 0.0 <= lams[0] <= 1.0
        if lams[0] == 1.0:
            assert np.array_equal(perms[0], ident)       # an unmixed step: lam = 1 and the identity
        else:
            mixed += 1
    assert 8 <= mixed <= 32                                # mixup_prob = 0.5 over 40 steps
    always, never = _head(_cfg(mixup_alpha=0.2, mixup_prob=1.0, mixup_mode="per_modality")), _head(_cfg(mixup_alpha=0.2, mixup_prob=0.0))
    for _ in range(10):
        lams, perms = always.draw(B)
        assert lams.shape == (4,) and perms.shape == (4, B) and len(set(lams)) == 4 and all(sorted(p) == list(ident) for p in perms)
        lams, perms = never.draw(B)
        assert lams[0] == 1.0 and np.array_equal(perms[0], ident)
    # Beta(0.2, 0.2) piles up at the ends: most draws are outside [0.1, 0.9]
    lam = np.array([always.draw(B)[0] for _ in range(200)]).ravel()
    assert ((lam < 0.1) | (lam > 0.9)).mean() > 0.4 and abs(lam.mean() - 0.5) < 0.1
    # an injected draw replaces the generator
    always.draw_source = lambda n: (np.array([0.25, 0.5, 0.75, 1.0]), np.tile(ident[::-1], (4, 1)))
    lams, perms = always.draw(B)
    assert list(lams) == [0.25, 0.5, 0.75, 1.0] and np.array_equal(perms[2], ident[::-1])


def test_cli_flags_parse():
    import run_train_eval as R
    argv = sys.argv
    try:
        sys.argv = ["run_train_eval.py"]
        a = R.parse_args()
        assert (a.criterion, a.focal_alpha, a.focal_gamma, a.mixup_alpha, a.mixup_prob, a.mixup_mode, a.warm_restarts) == \
            ("ce", 1.0, 2.0, 0.0, 0.5, "shared", None) and R.warm_restarts_arg(a.warm_restarts) is None
        sys.argv = ["run_train_eval.py", "--criterion", "focal", "--focal_gamma", "3.5", "--focal_alpha", "0.25", "--mixup_alpha", "0.2", "--mixup_prob", "0.75",
                    "--mixup_mode", "per_modality", "--warm_restarts", "5", "2", "1e-6"]
        a = R.parse_args()
        assert (a.criterion, a.focal_alpha, a.focal_gamma, a.mixup_alpha, a.mixup_prob, a.mixup_mode) == ("focal", 0.25, 3.5, 0.2, 0.75, "per_modality")
        assert R.warm_restarts_arg(a.warm_restarts) == (5, 2, 1e-6)
        for bad in (["--criterion", "bce"], ["--mixup_mode", "each"], ["--warm_restarts", "5", "2"]):
            sys.argv = ["run_train_eval.py"] + bad
            with pytest.raises(SystemExit):
                R.parse_args()
    finally:
        sys.argv = argv


def test_restatement_matches_the_reference_fixture():
    """tests/golden/recipe.npz (the reference's own FocalLoss / mixup_criterion / mixup_data) against the float32 restatement, within
    the device bound plus the reference's own cancellation in 1 - exp(-ce); the fixture's mixup_data rows equal the two-product mirror
    bit for bit when 1 - lam is formed in double and rounded once."""
    from tests.helpers import load_npz
    z = load_npz("recipe.npz")
    assert [tuple(r) for r in z["focal/alpha_gamma"]] == list(F.ALPHA_GAMMA) and set(np.abs(z["focal/gap"])) == set(np.abs(F.GAPS))
    lg, ya, yb, m = z["focal/logits"], z["focal/labels_a"], z["focal/labels_b"], z["focal/moderate"]
    assert (np.abs(z["focal/gap"][m]) <= 12).all() and len(m) == 21
    worst = {}
    for k, (alpha, gamma) in enumerate(F.ALPHA_GAMMA):
        for mixed in (False, True):
            mix = F.mix_of(float(z["focal/lam"])) if mixed else None
            a = F.focal_f32(lg, ya, yb if mixed else None, mix, alpha, gamma)
            b = F.focal_f32(lg[m], ya[m], yb[m] if mixed else None, mix, alpha, gamma)
            for key, r in F.fixture_checks(z, k, a["loss_rows"], float(a["loss"][0]), b["d_logits"], mixed).items():
                worst[key] = max(worst.get(key, 0.0), r)
    print("restatement against the reference fixture, error / (device bound + reference error):", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    x, lam, index = z["mixup/x"], float(z["mixup/lam"]), z["mixup/index"]
    mix = F.mix_of(lam)
    assert np.array_equal((mix[0] * x + mix[1] * x[index]).view(np.uint32), z["mixup/mixed"].view(np.uint32))
    assert np.array_equal(z["mixup/y"][index], z["mixup/y_b"]) and sorted(index) == list(range(len(index)))
