"""CPU checks of tests/graph_ops_cases.py: the suite of tests/test_gpu_graph_ops.py can see what it claims to see.

  * the float32 restatement of every entry stays inside its bound on every case, is bit-equal on the exact families, and alone
    keeps the ReLU-kink exclusions under the cap (in fact at none);
  * every mutant leaves a bound by MUTANT_FACTOR on at least one case; A_norm in place of A_norm^T is caught on the directed
    graphs and stays INSIDE the bound on every symmetric one, which is why no earlier test saw it;
  * the negative controls of the two dropout sites (the next step's masks, a row stride of hid + 4, the next layer's tag) put
    at least a quarter of the elements outside the bound;
  * the case table reaches every class the kernels distinguish.
References are computed once per (entry, case) and shared."""
import functools
import math

import numpy as np
import pytest

from tests import graph_ops_cases as G

OPS = sorted(G.OPS)


@functools.lru_cache(maxsize=None)
def _inp_ref(op, i):
    case = G.OPS[op].cases[i]
    inp = G.OPS[op].make(case)
    return inp, G.reference(op, case, inp)


def _restated(op, i, mutant=None):
    case = G.OPS[op].cases[i]
    inp, refs = _inp_ref(op, i)
    got = G.OPS[op].restate(case, inp, G.F32, mutant, G.case_muls(op, case))
    return case, refs, got


def ratios(op, mutant=None, select=None):
    """{case: worst error / bound over the outputs} of the float32 restatement (or a mutant of it)."""
    out = {}
    for i, case in enumerate(G.OPS[op].cases):
        if select is not None and not select(case):
            continue
        case, refs, got = _restated(op, i, mutant)
        out[case] = max(G.check(op, case, got, refs).values())
    return out


@pytest.mark.parametrize("op", OPS)
def test_fp32_restatement_stays_inside_the_bound(op):
    r = ratios(op)
    worst = max(r, key=r.get)
    print(f"{op}: restatement worst error / bound {r[worst]:.3g} at {G.case_id(worst)}")
    assert r[worst] <= 1.0, (op, worst, r[worst])
    for case, v in r.items():
        if G.is_exact(op, case):
            assert v == 0.0, (op, case, v)


def test_pretrain_loss_of_the_restatement_over_the_table():
    refs = [_inp_ref("gcn_pretrain", i)[1] for i in range(len(G.OPS["gcn_pretrain"].cases))]
    own = [r["_loss"][1] for r in refs]
    assert abs(G.loss_table_ratio(own, refs) - 1.0 / G.BOUND_FACTOR) < 1e-12
    assert all(math.isfinite(x) and x > 0 for x in own)
    wrong = list(own)
    wrong[3] = own[3] * (1 + 1e-4)
    assert G.loss_table_ratio(wrong, refs) >= G.MUTANT_FACTOR


def test_relu_kink_exclusions_stay_under_the_cap():
    worst = 0.0
    for i, case in enumerate(G.OPS["gnn"].cases):
        _, refs = _inp_ref("gnn", i)
        f = G.excluded_fraction(case, refs)
        worst = max(worst, f)
        assert f <= G.KINK_CAP, (case, f)
        if G.is_exact(op="gnn", case=case):
            assert f == 0.0, case
    print(f"gnn: largest excluded share of a case's gradient elements {worst:.4f} (cap {G.KINK_CAP})")


@pytest.mark.parametrize("op,mutant", [(op, m) for op in OPS for m in G.OPS[op].mutants])
def test_mutant_is_caught(op, mutant):
    r = ratios(op, mutant)
    best = max(r, key=r.get)
    print(f"{op} / {mutant}: best error / bound {r[best]:.3g} at {G.case_id(best)}; caught on {sum(v >= G.MUTANT_FACTOR for v in r.values())} of {len(r)} cases")
    assert r[best] >= G.MUTANT_FACTOR, (op, mutant, best, r[best])


@pytest.mark.parametrize("op", ("gnn", "gcn_pretrain"))
def test_untransposed_adjacency_is_seen_on_directed_graphs_only(op):
    r = ratios(op, "an_not_transposed", select=lambda c: c[6] in ("normal", "step1", "dropout"))
    sym = {c: v for c, v in r.items() if c[1] in G.SYMMETRIC}
    directed = {c: v for c, v in r.items() if c[1] in G.DIRECTED and c[0] > 2}
    print(f"{op}: A_norm for A_norm^T: symmetric worst {max(sym.values()):.3g}, directed smallest {min(directed.values()):.3g} (N > 2)")
    assert max(sym.values()) <= 1.0, max(sym, key=sym.get)
    assert min(directed.values()) >= G.MUTANT_FACTOR, min(directed, key=directed.get)
    assert len(sym) >= 6 * len(G.GRAPH_N) and len(directed) >= 3 * (len(G.GRAPH_N) - 2)


def test_designated_catchers():
    """The edge values are there because a named mutant needs them."""
    see = lambda op, m, sel: max(ratios(op, m, select=sel).values()) >= G.MUTANT_FACTOR
    assert see("gnn", "relu_ge_zero", lambda c: c[6] == "relu_zero")
    assert see("gnn", "pad_rows_not_zeroed", lambda c: c[0] == 33) and not see("gnn", "pad_rows_not_zeroed", lambda c: c[0] in (32, 64))
    assert see("gcn_pretrain", "adamw_decoupled_decay", lambda c: c[6] == "weight_decay")
    assert not see("gcn_pretrain", "adamw_decoupled_decay", lambda c: c[6] != "weight_decay")
    assert see("gcn_pretrain", "target_over_adj_plus_I", lambda c: c[1] == "empty")
    assert see("tcn", "one_pass_variance", lambda c: c[8] == "offset")
    assert see("tcn", "max_starts_at_zero", lambda c: c[8] == "negative")
    assert see("tcn", "running_var_biased", lambda c: c[7] == "train" and c[5] * c[6] in (2, 3))
    assert see("tcn", "right_heavy_padding", lambda c: c[3] in (2, 4)) and not see("tcn", "right_heavy_padding", lambda c: c[3] % 2 == 1 and c[7] == "eval")
    assert see("tcn", "taps_wrap_into_the_next_clip", lambda c: c[6] > 1 and c[3] > 1)
    assert not see("tcn", "taps_wrap_into_the_next_clip", lambda c: c[6] == 1)
    tiny = lambda c: c[2] >= 4
    assert see("temporal_align", "cosine_max_eps", tiny) and not see("temporal_align", "cosine_max_eps", lambda c: c[2] == 1)
    assert see("temporal_align", "visual_not_truncated_in_cosine", lambda c: c[1] > c[0])
    assert see("node_features", "norm_max_eps", lambda c: c[1] >= 4) and not see("node_features", "norm_max_eps", lambda c: c[1] == 1)


@pytest.mark.parametrize("op", ("gnn", "tcn"))
def test_dropout_negative_controls_leave_the_bound(op):
    """The float64 reference run with the wrong masks is outside the bound of the right ones on at least a quarter of the elements."""
    n = 0
    for i, case in enumerate(G.OPS[op].cases):
        if G.case_muls(op, case) is None:
            continue
        n += 1
        inp, refs = _inp_ref(op, i)
        hid = case[3] if op == "gnn" else case[2]
        controls = {"next step": dict(step=G.DROP_STEP + 1), "row stride hid + 4": dict(ld=hid + 4)}
        if op == "tcn":
            controls["next layer's tag"] = dict(shift=1)
        else:
            controls["the GCN's tag"] = dict(tag=9)
        for what, kw in controls.items():
            bad = G.OPS[op].restate(case, inp, G.F64, None, G.case_muls(op, case, **kw))
            for k in ("z", "g_w1", "g_w2") if op == "gnn" else ("out",):
                frac = G.outside_fraction(bad[k], *refs[k])
                print(f"{op} {G.case_id(case)} control {what}: {k} outside the bound on {frac:.3f}")
                assert frac >= 0.25, (case, what, k, frac)
    assert n >= 2


def test_exact_families_are_whole_numbers_and_relu_zero_is_zero():
    for i, case in enumerate(G.OPS["gnn"].cases):
        if not G.is_exact("gnn", case):
            continue
        inp, refs = _inp_ref("gnn", i)
        for k in ("z", "g_w1", "g_b1", "g_w2", "g_b2"):
            ref = refs[k][0]
            assert np.array_equal(ref, np.round(ref)) and np.abs(ref).max() < 2 ** 24 and not refs[k][1].any(), (case, k)
        if case[6] == "relu_zero":
            assert not refs["g_w1"][0].any() and not refs["g_b1"][0].any() and not refs["g_w2"][0].any() and refs["g_b2"][0].any()
            assert np.array_equal(refs["z"][0], np.broadcast_to(inp["b2"].astype(np.float64), refs["z"][0].shape))
        else:
            assert refs["g_w1"][0].any() and refs["z"][0].any()


def test_saturated_head_is_exact():
    for i, case in enumerate(G.OPS["gcn_pretrain"].cases):
        if not case[6].startswith("saturated"):
            continue
        case, refs, got = _restated("gcn_pretrain", i)
        for k in G.GCN_EXACT_OUTPUTS:
            assert not refs[k][1].any(), (case, k)
        assert not got["exp_avg"].any() and not got["exp_avg_sq"].any() and math.isfinite(float(got["loss"][0]))


def test_table_reaches_every_class():
    for op in ("gnn", "gcn_pretrain"):
        cases = G.OPS[op].cases
        normal = [c for c in cases if c[6] in ("normal", "step1")]
        assert {(c[0], c[1]) for c in normal} == {(n, k) for n in G.GRAPH_N for k in G.KINDS}
        assert G.GRAPH_N == (1, 2, 31, 32, 33, 64, 65, 257) and len(G.KINDS) == 9
        for n in G.GRAPH_N:
            mine = [c for c in normal if c[0] == n]
            assert {c[2] for c in mine} == {4, 20} and {c[3] for c in mine} == {32, 96} and {c[5] for c in mine} == {0, 3}, n
        for k in G.KINDS:
            mine = [c for c in normal if c[1] == k]
            assert {c[5] for c in mine} == {0, 3} and {c[3] for c in mine} == {32, 96}, k
        assert {c[4] for c in cases} == {32}
    assert {c[0] for c in G.OPS["gnn"].cases if c[6] == "exact"} == set(G.GRAPH_N)
    assert {(c[0], c[1] in G.DIRECTED) for c in G.OPS["gnn"].cases if c[6] == "dropout"} == {(33, False), (33, True), (64, False), (64, True)}
    assert {c[6] for c in G.OPS["gcn_pretrain"].cases} == set(G.GCN_VARIANTS)
    # graphs: a hub of degree N - 1, isolated nodes, a unit and a zero diagonal, weights in (0, 1], asymmetry
    a = G.make_adj("star", 33, 1)
    assert a[0].sum() == 32 and (a[1:].sum(axis=1) == 1).all()
    assert np.trace(G.make_adj("unit_diag", 33, 1)) == 33 and np.trace(G.make_adj("zero_diag", 33, 1)) == 0
    assert (G.make_adj("zero_diag", 257, 1).sum(axis=1) == 0).any() or (G.make_adj("empty", 257, 1).sum() == 0)
    w = G.make_adj("weighted_sym", 65, 1)
    assert np.array_equal(w, w.T) and w.max() <= 1 and w[w > 0].min() > 0 and len(np.unique(w)) > 10
    for k in G.DIRECTED:
        d = G.make_adj(k, 33, 1)
        assert not np.array_equal(d, d.T) and not np.trace(d), k
    assert G.make_adj("ring_directed", 33, 1).sum() == 33
    # node features
    nf = G.OPS["node_features"].cases
    assert {c[0] for c in nf} == {(1, 1, 1, 1), (3, 5, 7, 2), (192, 64, 96, 64)} and {c[1] for c in nf} == {1, 4, 5}
    inp, refs = _inp_ref("node_features", nf.index(((3, 5, 7, 2), 5)))
    assert not refs["out"][0][1].any() and not refs["out"][1][1].any() and refs["out"][0][0].any()
    assert abs(np.linalg.norm(refs["out"][0][2]) - 1 / 11) < 1e-3            # |v| = 1e-10: v / (|v| + 1e-9) has norm 1 / 11
    # temporal align: every D; Dv below, at and above D and Dv = 1; every B; every row kind; the pad of 4 D + 1
    ta = G.OPS["temporal_align"].cases
    assert {c[0] for c in ta} == {1, 2, 3, 64, 65} and {c[2] for c in ta} == {1, 4, 5}
    for D in G.TA_D:
        dv = {c[1] for c in ta if c[0] == D}
        assert 1 in dv and D in dv and any(x > D for x in dv) and (D == 1 or any(x < D for x in dv)), D
        assert (-(4 * D + 1)) % 4 == 3
    assert set(G.ta_row_kinds(5)) | set(G.ta_row_kinds(4)) == set(G.TA_ROWS)
    i = ta.index((64, 64, 5))
    inp, _ = _inp_ref("temporal_align", i)
    cos = G.OPS["temporal_align"].restate(ta[i], inp, G.F32)["_cos"]
    kinds = G.ta_row_kinds(5)
    assert all(cos[r] == 0.0 for r, k in enumerate(kinds) if "zero" in k) and abs(cos[kinds.index("identical")] - 1) < 1e-6
    assert 0 < abs(cos[kinds.index("tiny")]) < 0.02                            # (1e-10 / 1.1e-9)^2 |cos|: the eps decides
    # TCN
    tc = G.OPS["tcn"].cases
    assert {(c[0], c[1]) for c in tc} == {(3, 2), (16, 16), (40, 24)} and {c[2] for c in tc} == {32, 96}
    assert {c[3] for c in tc} == {1, 2, 3, 4, 15} and {c[4] for c in tc} == {1, 4, 6} and {c[5] for c in tc} == {1, 2, 5, 33} and {c[6] for c in tc} == {1, 3}
    assert {c[5] * c[6] for c in tc if c[7] == "train"} >= {2, 3} and {c[8] for c in tc} == {None, "negative", "constant", "offset"}
    assert any(c[0] + c[1] == c[2] for c in tc) and any(c[0] + c[1] > c[2] for c in tc) and any((c[0] + c[1]) * c[3] % 4 for c in tc)
    assert any(c[7] == "dropout" and c[4] == 6 for c in tc)                    # tag 16 + 5 = 21
    assert any(c[5] == 5 and c[4] == 4 and c[3] == 3 for c in tc)              # T = 5, dilations 4 and 8: off-centre taps outside the clip
    i = [c[8] for c in tc].index("constant")
    inp, refs = _inp_ref("tcn", i)
    assert not inp["layers"][0]["w"][5].any()
    i = [c[8] for c in tc].index("negative")
    # adjacency
    for n in G.ADJ_N:
        sets = G.adjacency_sets(n)
        assert len(sets) == n and len(sets[0]) == 2048 and len(sets[1]) == 2049 and not sets[5]
        a, w = G.adjacency_refs(sets[:8], G.ADJ_THRESH)
        assert a[3, 4] == 0 and w[3, 4] == np.float32(1 / 3) and a[0, 1] == 1 and w[0, 2] > 0
