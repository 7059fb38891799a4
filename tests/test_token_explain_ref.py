"""CPU: the yardstick of the token / image-patch attributions (tests/token_explain_ref.py) against the oracle it is built on, and
explain.input_attribution's refusal to run anywhere but on a HIP device."""
import pytest
import torch

from oracle import encoders_ref as E
from oracle import tier_a as O
from tests import token_explain_ref as R


def _text(B=3, Lq=20, seed=5):
    w = E.seeded_weights(E.bert_shapes(layers=2, vocab=300), seed)
    ids, mask = E.synthetic_tokens(seed + 1, B, Lq, vocab=300, min_len=4)
    ids[0, 3] = ids[0, 1]                     # a repeated id inside a sample and across samples: the scatter has to add
    ids[1, 2] = ids[0, 1]
    return w, ids, mask


def test_gathered_table_reproduces_the_oracle_features_exactly():
    w, ids, mask = _text()
    wl, pos_ids = R.gathered(w, ids, torch.float32)
    assert wl[R.WORD].shape == (ids.numel(), 768) and torch.equal(pos_ids.reshape(-1), torch.arange(ids.numel()))
    assert torch.equal(E.text_features(wl, pos_ids, mask), E.text_features(w, ids, mask))


def test_gathered_gradient_scattered_by_id_is_the_oracle_word_table_gradient():
    w, ids, mask = _text()
    w64 = {k: v.double() for k, v in w.items()}
    _, ref = E.text_feature_grads(w64, ids, mask, seed=9)
    dfeat = torch.randn(ids.shape[0], 768, generator=torch.Generator().manual_seed(9))
    feat, g = R.text_input_grad(w, ids, mask, dfeat)
    assert g.dtype == torch.float64 and g.shape == (ids.numel(), 768)
    scattered = torch.zeros_like(ref[R.WORD]).index_add_(0, ids.reshape(-1), g)
    err = (scattered - ref[R.WORD]).abs().max().item()
    print(f"scattered per-position gradient vs the oracle's word-table gradient: max |diff| {err:.2e} of {ref[R.WORD].abs().max().item():.2e}")
    assert err <= 1e-12 * ref[R.WORD].abs().max().item() + 1e-18
    assert (g.view(*ids.shape, -1)[mask == 0] == 0).all()          # masked positions carry no gradient


def _case(B=2, Lq=12, Fr=1, seed=40):
    wt = E.seeded_weights(E.bert_shapes(layers=2, vocab=300), seed)
    wv = E.seeded_weights(E.vit_shapes(layers=2), seed + 1)
    ids, mask = E.synthetic_tokens(seed + 2, B, Lq, vocab=300, min_len=4)
    batch = dict(O.seeded_batch(seed + 3, B))
    batch.update({"input_ids": ids, "attention_mask": mask, "frames": E.synthetic_frames(seed + 4, B, Fr)})
    del batch["text_features"], batch["visual_features"]
    return wt, wv, batch


def test_integrated_gradients_sum_approaches_delta_as_steps_double():
    """Completeness: the sum of all token and pixel scores of a sample approaches delta = logit(input) - logit(baselines) as the
    midpoint rule's steps double, 8 -> 16 -> 32: the worst sample's error does not increase.  The error does not go to zero: the
    head's evidence scalars carry no gradient (oracle.tier_a.fusion_forward, as the reference: `no_grad`), so what they contribute
    to delta along the path is attributed to nobody; that gap and the kinks of |t - a| in the pair features are why the batch's
    worst error is watched (B = 4), not every sample's own."""
    wt, wv, batch = _case(B=4, Lq=8, seed=60)
    fus, clf = ({k: v.double() for k, v in sd.items()} for sd in O.seeded_params(1234))
    errs = []
    for steps in (8, 16, 32):
        r = R.input_attribution(fus, clf, wt, wv, batch, method="integrated_gradients", steps=steps)
        total = r["tokens"].sum(1) + r["pixels"].flatten(1).sum(1)
        assert torch.allclose(r["patches"].flatten(1).sum(1), r["pixels"].flatten(1).sum(1), rtol=1e-9, atol=1e-12)
        errs.append((total - r["delta"]).abs().max().item())
    print(f"|sum of attributions - delta| at 8 / 16 / 32 steps: {errs[0]:.3e} / {errs[1]:.3e} / {errs[2]:.3e} (delta {r['delta'].tolist()})")
    assert errs[0] >= errs[1] >= errs[2]
    assert errs[2] < r["delta"].abs().max().item()


def test_grad_x_input_is_the_one_step_gradient_at_the_input():
    wt, wv, batch = _case(B=2, Lq=8)
    fus, clf = ({k: v.double() for k, v in sd.items()} for sd in O.seeded_params(1234))
    r = R.input_attribution(fus, clf, wt, wv, batch, class_idx=0)
    assert r["tokens"].shape == (2, 8) and r["patches"].shape == (2, 1, 49) and r["pixels"].shape == (2, 1, 3, 224, 224)
    assert (r["tokens"][batch["attention_mask"] == 0] == 0).all() and (r["token_grad_norm"] >= 0).all()
    assert (r["tokens"].abs() <= r["token_scale"][:, None] * (1 + 1e-12)).all()          # Cauchy-Schwarz, token by token


def test_input_attribution_on_cpu_modules_raises():
    from ultrafnd_git_amd import _lib as L
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.explain import input_attribution
    from ultrafnd_git_amd.fusion import CrossModalTransformer
    fusion, clf = CrossModalTransformer(), DeepTruthClassifier()
    tenc, venc = BertTextEncoder(layers=1, vocab_size=50), ClipVisualEncoder(layers=1)
    _, _, batch = _case(B=1, Lq=4)
    with pytest.raises(L.UltrafndHipError, match="HIP device only"):
        input_attribution(fusion, clf, tenc, venc, batch)
    for bad in (dict(class_idx=2), dict(method="shap"), dict(method="integrated_gradients", steps=0)):
        with pytest.raises(ValueError):
            input_attribution(fusion, clf, tenc, venc, batch, **bad)
