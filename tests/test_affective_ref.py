"""CPU: the yardsticks of tests/test_gpu_affective.py, and the affective C entries' argument checks.

  - the restated position-id rule equals HF's create_position_ids_from_input_ids; the bf16=False mirror is the HF model itself
  - the float64 head restatement reproduces tests/golden/affective.npz (the real reference's analyze) inside the derived bound
  - the group table from the default names and from names that hit several rules
  - every new entry refuses a bad call with rc == 1 and a ufnd_last_error text, before any launch"""
import numpy as np
import pytest
import torch

from tests import affective_ref as R

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def test_position_ids_equal_hfs_function():
    from transformers.models.roberta import modeling_roberta as MR
    hf = getattr(MR, "create_position_ids_from_input_ids", None) or MR.RobertaEmbeddings.create_position_ids_from_input_ids
    cases = [R.make_batch((5, 12, 0, 1), 12, seed=1),                                   # pads at the end, none, everywhere, <s> alone
             R.make_batch((9, 12, 7), 12, seed=2, holes=((0, 3), (1, 5), (1, 6))),      # pads in the middle
             R.make_batch((130, 64, 65), 130, seed=3, holes=((0, 64), (2, 63)))]        # across the 64-token chunks of the kernel's scan
    for ids, _ in cases:
        for pad in (1, 0, 3):
            assert torch.equal(R.position_ids(ids, pad), hf(ids, pad)), pad
    ids, _ = cases[1]
    assert R.position_ids(ids)[0].tolist() == [2, 3, 4, 1, 5, 6, 7, 8, 9, 1, 1, 1]


def test_mirror_without_rounding_is_hf():
    from ultrafnd_git_amd.affective import RobertaEmotionClassifier
    sd = R.case_weights(RobertaEmotionClassifier(num_hidden_layers=2, vocab_size=R.VOCAB).state_dict())
    ids, mask = R.make_batch((9, 16, 1, 5), 16, seed=4, holes=((0, 4),))
    ref = R.reference(R.hf_model(sd, 2), ids, mask)
    for form in R.FORMS:
        got = R.mirror(sd, ids, mask, 2, bf16=False, form=form)
        for k in ("embed", "logits", "class_probs"):
            assert torch.allclose(got[k], ref[k], rtol=0, atol=1e-11), (form, k)
        for a, b in zip(got["layers"], ref["layers"]):
            assert torch.allclose(a, b, rtol=0, atol=1e-11), form
    # with rounding every form is a small, positive distance away: "3 x the mirror" means something
    for form in R.FORMS:
        m = R.mirror(sd, ids, mask, 2, form=form)
        for got, want in ((m["layers"][-1], ref["layers"][-1]), (m["logits"], ref["logits"])):
            assert not R.mirror_within_sanity(got, want), (form, R.mirror_within_sanity(got, want))


def _geometry_params(kind):
    from tests import encoder_geometry_cases as G
    return [pytest.param(c, id=c.id) for c in (G.ROBERTA_CASES if kind == "roberta" else G.BERT_CASES)]


@pytest.mark.parametrize("c", _geometry_params("roberta") + _geometry_params("bert"))
def test_mirror_at_every_geometry_of_the_table(c):
    """tests/encoder_geometry_cases.py: RoBERTa and BERT at the four widths, L = 40 and 128, in the form the encoder takes there (read
    from the encoder: at hidden 1024 the unfolded fallback).  With the roundings off the mirror is the float64 yardstick -- HF's
    RobertaForSequenceClassification at that geometry, oracle/encoders_ref in float64 for BERT -- and with them on it stays inside the
    sanity band on every input of tests/test_gpu_encoder_geometry.py."""
    from tests import encoder_geometry_cases as G
    form = G.form_of(G.text_encoder(c), len(c.lengths), c.L)["form"]
    assert form in R.FORMS
    ref, exact = G.text_ref_mirror(c, form, False)
    for name, got, want in G.stages(ref, exact) + [("embed", exact["embed"], ref["embed"])]:
        assert torch.allclose(got, want, rtol=0, atol=1e-11), (form, name)
    _, mir = G.text_ref_mirror(c, form)
    for name, got, want in G.stages(ref, mir):
        if name == "class_probs" and c.labels == 1:      # softmax over one label is the constant 1: nothing rounds, the GPU is held to it exactly
            assert torch.equal(got, want) and bool((want == 1).all())
            continue
        assert not R.mirror_within_sanity(got, want), (form, name, R.mirror_within_sanity(got, want))


@pytest.mark.parametrize("hidden,form", [(256, "folded-fp32"), (1024, "unfolded")])
def test_encode_fields_mirror_at_the_tables_widths(hidden, form):
    """encode_fields' input of tests/test_gpu_encoder_geometry.py (strict: the fp32 stream; unfolded at 1024): exact without roundings,
    inside the sanity band with them; the record without parts is a zero row in both."""
    from tests import encoder_geometry_cases as G
    ref, exact = G.fields_ref_mirror(hidden, form, False)
    assert torch.allclose(exact, ref, rtol=0, atol=1e-11) and not ref[2].any() and not exact[2].any()
    assert torch.allclose(ref[:2].norm(dim=-1), torch.ones(2, dtype=torch.float64), atol=1e-8)
    _, mir = G.fields_ref_mirror(hidden, form)
    assert not R.mirror_within_sanity(mir[:2], ref[:2]), R.mirror_within_sanity(mir[:2], ref[:2])


def test_head_restatement_reproduces_the_reference(golden_dir):
    z = np.load(golden_dir / "affective.npz")
    names = [str(n) for n in z["labels"]]
    assert tuple(names) == R.DEFAULT_LABELS
    lens, off, ar, ar_err = z["clip_lengths"], 0, [], []
    for n in lens:
        clip = z["clips"][off:off + max(n, 0)]
        off += max(n, 0)
        ar.append(0.5 if n < 0 else R.arousal_ref(clip))
        ar_err.append(0.0 if n < 0 else R.arousal_bound(clip))
    assert off == z["clips"].shape[0]
    got = R.post_ref(z["logits"], names, valid=z["text_valid"], arousal=ar)
    # float64 against the reference, whose softmax and group sums are float32 (torch.softmax on float32 logits, p[...].sum()) and the
    # rest float64 -- head_bounds' softmax and group terms: rp = (range + C + 5) eps relative per probability, C eps per group sum, twice
    # for the quotient
    C = len(names)
    rng = float((z["logits"].max(-1) - z["logits"].min(-1)).max())
    # (its np.mean(audio ** 2) is float32 too: a rounded square per sample, numpy's pairwise sum -- runs of at most 128 terms in eight
    #  interleaved chains, then a tree -- and the division: <= (1 + 16 + 3 + log2(n) + 1) eps of the mean, through sigmoid(5 m)'s slope 5 / 4)
    en = max(float(np.mean(z["clips"][a:b].astype(np.float64) ** 2)) for a, b in zip(np.cumsum(np.maximum(lens, 0)) - np.maximum(lens, 0),
                                                                                         np.cumsum(np.maximum(lens, 0))) if b > a)
    bounds = {"probs": 2 * ((rng + C + 5) * R.EPS32 + C * R.EPS32) + 1e-15,
              "arousal": 1.25 * en * (21 + np.log2(max(lens))) * R.EPS32 + 1e-15}
    bounds["intensity"] = 0.6 * 0.625 * 2 * bounds["probs"] + 0.4 * bounds["arousal"] + 1e-15
    bounds["valence"] = bounds["probs"] + 1e-15
    for k, bound in bounds.items():
        err = float((got[k] - torch.from_numpy(z["out/" + k])).abs().max())
        print(f"AFFECTIVE_ERR ref_vs_golden {k} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    empty = int(np.flatnonzero(z["text_valid"] == 0)[0])
    assert got["probs"][empty].tolist() == [0.0, 0.0, 0.0] and float(got["text_intensity"][empty]) == 0.5
    assert max(ar_err) < 1e-5      # the arousal bound is a rounding bound, not a tolerance


def test_group_table():
    from ultrafnd_git_amd.affective import DEFAULT_ID2LABEL, AffectiveForensics, group_table  # noqa: F401
    assert DEFAULT_ID2LABEL == R.DEFAULT_LABELS
    assert group_table(DEFAULT_ID2LABEL) == [1, -1, 0, 2, -1, -1, -1] == R.group_table(R.DEFAULT_LABELS)
    multi = ["Fearful RAGE", "worried", "madly happy", "amusement", "scared annoyed delight", "LABEL_5", "happiness"]
    assert group_table(multi) == [4 + 3, 0, 1, 2, 4 + 7, -1, 2] == R.group_table(multi)      # "happy" has no "happi"
    gm = R.group_masks(multi)
    assert gm[:, 0].tolist() == [1, 1, 0] and gm[:, 4].tolist() == [1, 1, 1] and gm[:, 5].tolist() == [0, 0, 0]


def test_entries_refuse_bad_arguments():
    lib = _lib()
    err = lib.ufnd_last_error
    # ufnd_roberta_embed[_live]: L = 513 with 514 positions and pad 1 (position ids would run to 514); H; nulls
    embed = lambda L=128, H=768, ids=P, out=P: lib.ufnd_roberta_embed(ids, P, P, P, P, P, P, out, None, 2, L, H, 300, 514, 1, 1e-5, None)
    assert embed(L=513) == 1 and b"L=513" in err()
    assert embed(H=770) == 1 and b"H=770" in err()
    assert embed(ids=None) == 1 and b"null" in err()
    assert embed(out=None) == 1 and b"null" in err()
    live = lambda L=128, H=768, row_src=P: lib.ufnd_roberta_embed_live(P, P, row_src, P, P, P, P, P, P, P, None, 256, L, H, 300, 514, 1, 1e-5, None)
    assert live(L=513) == 1 and b"L=513" in err()
    assert live(H=100) == 1 and b"H=100" in err()
    assert live(row_src=None) == 1 and b"null" in err()
    # ufnd_roberta_pack
    assert lib.ufnd_roberta_pack(None, P, 2, 16, 1, P, P, P, P, None) == 1 and b"null" in err()
    assert lib.ufnd_roberta_pack(P, P, 2, 16, 1, P, None, P, P, None) == 1 and b"null" in err()      # cu without row_src
    assert lib.ufnd_roberta_pack(P, P, 16385, 16, 1, None, None, P, None, None) == 1 and b"B=16385" in err()
    assert lib.ufnd_roberta_pack(P, P, 2, 16, -1, None, None, P, None, None) == 1 and b"pad=-1" in err()
    # ufnd_gather_class_rows
    gather = lambda H=768, ctx=(P, P), st=(None, None), sf=0, B=2, cap=32: lib.ufnd_gather_class_rows(None, *ctx, None, None, None, None, *st, B, 16, H, sf,
                                                                                                       cap, None)
    assert gather(H=770) == 1 and b"H=770" in err()
    assert gather(ctx=(P, None)) == 1 and b"null" in err()
    assert gather(ctx=(None, None)) == 1 and b"null" in err()
    assert gather(st=(P, P), sf=0) == 1 and b"stat_floats=0" in err()
    assert gather(B=3) == 1 and b"capacity=32" in err()      # the padded rows b L must lie inside the sources
    # ufnd_emotion_head: C = 33, H not a multiple of 32, nulls, a partial output set
    head = lambda H=768, C=7, x=P, probs=(P, P, P, P), group=P: lib.ufnd_emotion_head(x, P, P, P, P, group, None, None, P, P, P, *probs, 4, H, C, None)
    assert head(C=33) == 1 and b"C=33" in err()
    assert head(C=0) == 1 and b"C=0" in err()
    assert head(H=770) == 1 and b"H=770" in err()
    assert head(H=2048) == 1 and b"H=2048" in err()
    assert head(x=None) == 1 and b"null" in err()
    assert head(probs=(P, None, P, P)) == 1 and b"go together" in err()
    assert head(group=None) == 1 and b"go together" in err()
    # ufnd_audio_arousal
    assert lib.ufnd_audio_arousal(None, None, P, 1, 16, None) == 1 and b"null" in err()
    assert lib.ufnd_audio_arousal(P, None, P, 1, 0, None) == 1 and b"T=0" in err()
    assert lib.ufnd_audio_arousal(P, None, P, 65536, 16, None) == 1 and b"B=65536" in err()


def test_classifier_refuses_by_name():
    from ultrafnd_git_amd._lib import UltrafndHipError
    from ultrafnd_git_amd.affective import AffectiveForensics, RobertaEmotionClassifier
    with pytest.raises(ValueError, match="num_labels=33"):
        RobertaEmotionClassifier(num_hidden_layers=1, vocab_size=R.VOCAB, num_labels=33)
    enc = RobertaEmotionClassifier(num_hidden_layers=1, vocab_size=R.VOCAB)
    assert list(enc.state_dict())[0] == "roberta.embeddings.word_embeddings.weight" and enc.state_dict()["roberta.embeddings.position_embeddings.weight"].shape[0] == 514
    sd = enc.state_dict()
    with pytest.raises(RuntimeError, match="unexpected keys"):
        enc.load_state_dict(dict(sd, **{"roberta.pooler.dense.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="missing keys"):
        enc.load_state_dict({k: v for k, v in sd.items() if not k.startswith("classifier.out_proj")})
    ids = torch.zeros(1, 513, dtype=torch.long)
    with pytest.raises(UltrafndHipError, match="HIP device only"):      # (no CPU path)
        enc.logits(ids[:, :16], torch.ones(1, 16))
    enc._require_hip = lambda: None
    with pytest.raises(RuntimeError, match="sequence length 513 exceeds"):
        enc.logits(ids, torch.ones_like(ids))
    with pytest.raises(ValueError, match="names 3 labels"):
        AffectiveForensics(classifier=enc, id2label=["a", "b", "c"], device="cpu")
