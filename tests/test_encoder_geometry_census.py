"""CPU: the geometry table of tests/test_gpu_encoder_geometry.py (tests/encoder_geometry_cases.py) still reaches every form of the
frozen encoders' passes.  The form of each case is read from the encoder's own dispatch (encoder_geometry_cases.form_of: the
statistics buffers _workbufs allocates after asking ufnd_gemm_bf16_stat_parts, _fuses, _cls_rows), so a change of the library's tile
choice, of the fold rule or of a fuse condition that moves the cases off a form fails here, and the cases have to be chosen again."""
import pytest

from tests import encoder_geometry_cases as G


def _forms(cases, build, shape):
    out = {}
    for c in cases:
        out[c.id] = (c, G.form_of(build(c), *shape(c)))
    return out


@pytest.fixture(scope="module")
def bert():
    return _forms(G.BERT_CASES, G.text_encoder, lambda c: (len(c.lengths), c.L))


@pytest.fixture(scope="module")
def roberta():
    return _forms(G.ROBERTA_CASES, G.text_encoder, lambda c: (len(c.lengths), c.L))


@pytest.fixture(scope="module")
def vit():
    return {f"{c.id}-B{B}F{Fr}": (c, G.form_of(G.vit_encoder(c), B, Fr)) for c in G.VIT_CASES for B, Fr in G.VIT_BATCHES}


def test_the_table_has_the_issues_widths_and_shapes():
    assert [w[0] for w in G.WIDTHS] == [256, 512, 768, 1024] and all(h == 64 * nh and it % 64 == 0 for h, nh, it in G.WIDTHS)
    assert G.WIDTHS[0][2] % 128 == 0 and G.WIDTHS[0][2] % 192 and G.WIDTHS[0][2] % 256      # 640: no multiple of the 192- and 256-wide tiles
    for cases in (G.BERT_CASES, G.ROBERTA_CASES):
        assert {(c.hidden, c.L) for c in cases} >= {(h, L) for h, _, _ in G.WIDTHS for L in (40, 128)}
        assert all(c.lengths == (1, 16, 17, c.L - 1, c.L) for c in cases)
    assert {c.labels for c in G.ROBERTA_CASES} == {1, 7, 32}
    assert {c.tokens for c in G.VIT_CASES if c.hidden == 768} == {2, 5, 17, 50, 65, 197}
    assert {(c.hidden, c.tokens) for c in G.VIT_CASES} >= {(256, 50), (512, 50), (1024, 50), (1024, 65), (256, 197)}
    assert 3 * G.VIT_TOKENS[17][0] ** 2 == 192 and {(c.hidden, c.proj) for c in G.VIT_CASES} >= {(256, 192), (512, 512), (1024, 1024)}
    assert {B * Fr for B, Fr in G.VIT_BATCHES} >= {1, 3} and (2, 2) in G.VIT_BATCHES
    assert {c.hidden for c in G.CLIP_TEXT_CASES if c.L == 77} == {256, 512, 768, 1024}
    assert all(c.e_list == (1, 15, 16, 63, 64, 76) for c in G.CLIP_TEXT_CASES if c.L == 77)
    long = {c.L: c for c in G.CLIP_TEXT_CASES if c.max_pos == 248}
    assert sorted(long) == [128, 129, 193, 248] and all(c.hidden == 512 for c in long.values())
    assert long[248].e_list == (127, 128, 191, 192, 247) and long[128].e_list == (127,) and long[193].e_list == (127, 128, 191, 192)
    assert all(len(b) <= 5 for c in G.CLIP_TEXT_CASES for b in c.batches)


@pytest.mark.parametrize("family", ("bert", "roberta"))
def test_text_cases_reach_every_form(family, request):
    forms = request.getfixturevalue(family)
    for name, (c, f) in forms.items():
        print(f"ENC_GEOM_FORM {name} {f}")
    at = lambda **kw: [f for c, f in forms.values() if all(getattr(c, k) == v for k, v in kw.items())]
    # folded with 8, 16 and 24 partials per row, at the widths that give them
    assert {(c.hidden, f["parts"]) for c, f in forms.values() if f["parts"]} == {(256, 8), (512, 16), (768, 24)}
    assert {f["form"] for f in at(hidden=768)} == {"folded-bf16", "folded-fp32", "unfolded"}
    # the unfolded fallback at 1024, under both residual dtypes (nobody asked for it: fold_ln is on)
    fallback = [(c, f) for c, f in forms.values() if c.hidden == 1024]
    assert all(c.fold_ln and f["form"] == "unfolded" and f["parts"] == 0 for c, f in fallback)
    assert {c.residual_dtype for c, _ in fallback} == {"bf16", "fp32"}
    # fused at L = 128 and two launches at L = 40, at every width
    for h, _, _ in G.WIDTHS:
        assert [f["fused"] for f in at(hidden=h, L=128)] == [True] and not any(f["fused"] for f in at(hidden=h, L=40))
    assert {f["ni"] for _, f in forms.values()} == {1, 2, 3, 4}
    if family == "roberta":      # the class-row tail over folded and over unfolded buffers
        assert {f["tail"] for _, f in forms.values()} == {"folded", "unfolded"}
        assert {f["tail"] for f in at(hidden=1024)} == {"unfolded"} and "folded" in {f["tail"] for f in at(hidden=256)}
    else:
        assert {f["tail"] for _, f in forms.values()} == {None}


def test_vit_cases_reach_every_form(vit):
    for name, (c, f) in vit.items():
        print(f"ENC_GEOM_FORM {name} {f}")
    assert {(c.hidden, f["parts"]) for c, f in vit.values() if f["parts"]} == {(256, 8), (512, 16), (768, 24)}
    assert {f["form"] for c, f in vit.values() if c.hidden == 768} == {"folded-bf16", "folded-fp32", "unfolded"}
    fallback = [(c, f) for c, f in vit.values() if c.hidden == 1024]
    assert all(c.fold_ln and f["form"] == "unfolded" for c, f in fallback) and {c.residual_dtype for c, _ in fallback} == {"bf16", "fp32"}
    # fused up to 64 tokens, two launches from 65 on: both at 768, 65 at 1024 and 197 at 256
    assert {c.tokens for c, f in vit.values() if f["fused"]} == {2, 5, 17, 50}
    assert {(c.hidden, c.tokens) for c, f in vit.values() if not f["fused"]} == {(768, 65), (768, 197), (1024, 65), (256, 197)}
    # the class-row tail over the statistics buffers and over the compact hc buffer, each with fused and with two-launch attention
    assert {(f["tail"], f["fused"]) for _, f in vit.values()} == {("folded", True), ("folded", False), ("unfolded", True), ("unfolded", False)}
    assert {f["ni"] for _, f in vit.values()} == {1, 2, 3, 4}
    # the form does not depend on the frame count: the three batches of a case agree
    for c in G.VIT_CASES:
        assert len({tuple(sorted(vit[f"{c.id}-B{B}F{Fr}"][1].items())) for B, Fr in G.VIT_BATCHES}) == 1, c.id


def test_the_librarys_tile_choice_avoids_192_wide_tiles_where_they_do_not_divide():
    """N = 256, 512, 1024 and 640 are no multiples of 192: whatever tile the library picks for the cases' GEMM shapes divides N (the plan
    entry of the diagnostics library reports the choice the product entry makes)."""
    from tools import _diaglib as D
    P = 1 << 12      # an aligned, never dereferenced address
    for h, _, it in ((h, nh, it) for h, nh, it in G.WIDTHS if h != 768):
        for M in (5, 3 * 50, 5 * 40, 5 * 128, 3 * 197):
            for N, K in ((3 * h, h), (h, h), (it, h), (h, it)):
                rc, p, err = D.gemm_bf16_plan("gemm", A=P, W=P, out_bf16=P, M=M, N=N, K=K, lda=K, ldw=K, ldo=N)
                assert rc == 0 and N % p["bn"] == 0 and (p["bn"] != 192 or N % 192 == 0), (M, N, K, p, err)
