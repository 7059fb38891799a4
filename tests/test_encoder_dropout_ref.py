"""CPU: the dropout restatement of the encoders (tests/encoder_dropout_ref.py) is pinned twice -- without masks to
oracle/encoders_ref.py, with masks to the installed third-party BertModel / CLIPVisionModelWithProjection in train mode, whose
dropout calls are answered from a queue of those masks in call order -- and the public surface of encoder dropout (constructor
arguments, TrainConfig.encoder_dropout) accepts p in [0, 1) and refuses the rest by name."""
import pytest
import torch

from oracle import encoders_ref as E
from tests import encoder_dropout_ref as R


def _close(a, b, rel):
    assert a.shape == b.shape
    err = (a - b).norm().item()
    assert err <= rel * max(b.norm().item(), 1e-30), (err, b.norm().item())


def _close_grads(got, ref, rel):
    """Every gradient tensor to `rel` relative L2, with an absolute floor of rel x 1e-2 of the largest one (the key bias's
    gradient is zero up to rounding, by softmax's shift invariance)."""
    top = max(r.norm().item() for r in ref.values())
    for k, r in ref.items():
        assert got[k].shape == r.shape, k
        err = (got[k] - r).norm().item()
        assert err <= rel * (r.norm().item() + 1e-2 * top), (k, err, r.norm().item())


def _text_case(layers=2, B=2, L=22):
    w = {k: v.double() for k, v in E.seeded_weights(E.bert_shapes(layers=layers, vocab=300), 61).items()}
    ids, mask = E.synthetic_tokens(62, B, L, vocab=300, min_len=5)
    return w, ids, mask


def test_restatement_without_masks_equals_the_oracle():
    w, ids, mask = _text_case()
    f0, g0 = E.text_feature_grads(w, ids, mask, 7)
    f1, g1 = R.text_feature_grads(w, ids, mask, 7, masks=None)
    assert f0.dtype == f1.dtype == torch.float64
    _close(f1, f0, 1e-13)
    for k in g0:
        _close(g1[k], g0[k], 1e-12)
    # ViT: encoders_ref casts the pixels with .float(), so this half runs in float32
    wv = E.seeded_weights(E.vit_shapes(layers=1), 63)
    frames = E.synthetic_frames(64, 2, 1)
    f0, g0 = E.visual_feature_grads(wv, frames, 8)
    f1, g1 = R.visual_feature_grads(wv, frames, 8, masks=None, dtype=torch.float32)
    _close(f1, f0, 1e-6)
    for k in g0:
        _close(g1[k], g0[k], 1e-5)


def test_masks_change_the_result_and_keep_about_nine_in_ten():
    w, ids, mask = _text_case()
    m = R.text_masks(5, 3, 2, 22, 2, p_hidden=0.1, p_attn=0.1)
    assert m[("attn", 0)].shape == (2, 12, 22, 22) and m["emb"].shape == (2, 22, 768)
    keep = torch.cat([v.flatten() for v in m.values()])
    assert set(torch.unique(keep).tolist()) == {0.0, float(torch.tensor(1.0) / (1.0 - torch.tensor(0.1)))}
    assert 0.88 <= (keep != 0).double().mean().item() <= 0.92
    f0, _ = R.text_feature_grads(w, ids, mask, 7)
    f1, _ = R.text_feature_grads(w, ids, mask, 7, masks=m)
    assert (f1 - f0).abs().max().item() > 1e-3
    # the attention site's numbering pads keys to a multiple of 4: at L = 22 element (q, k) is q * 24 + k
    from tests import dropout_mirror as DM
    u = DM.multipliers(5, 3, R.tag_text(1, "attn"), 0.1, 24, 24, 24)
    assert torch.equal(m[("attn", 1)][0, 0], torch.from_numpy(u[:22, :22]))


class _MaskQueue:
    """torch.nn.functional.dropout replaced: every call takes the next mask (and checks p)."""

    def __init__(self, masks, p):
        self.masks, self.p, self.calls = list(masks), p, 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        assert training and abs(p - self.p) < 1e-12, (p, training)
        m = self.masks[self.calls]
        self.calls += 1
        assert m.shape == x.shape, (m.shape, x.shape)
        return x * m.to(x.dtype)


def test_restatement_with_masks_equals_the_third_party_models_in_train_mode(monkeypatch):
    transformers = pytest.importorskip("transformers")
    layers, B, L, p = 2, 2, 22, 0.1
    w, ids, mask = _text_case(layers, B, L)
    masks = R.text_masks(11, 4, B, L, layers, p_hidden=p, p_attn=p)
    order = ["emb"] + [(s, i) for i in range(layers) for s in ("attn", "attn_out", "ffn_out")]
    cfg = transformers.BertConfig(num_hidden_layers=layers, vocab_size=300, hidden_dropout_prob=p, attention_probs_dropout_prob=p,
                                  attn_implementation="eager")
    m = transformers.BertModel(cfg, add_pooling_layer=False).double()
    m.load_state_dict(w, strict=True)
    m.train()
    q = _MaskQueue([masks[k] for k in order], p)
    monkeypatch.setattr(torch.nn.functional, "dropout", q)
    feat = E.masked_meanpool_l2(m(input_ids=ids, attention_mask=mask).last_hidden_state, mask)
    E.probe_loss(feat, 9).backward()
    monkeypatch.undo()
    assert q.calls == len(order)
    f1, g1 = R.text_feature_grads(w, ids, mask, 9, masks=masks)
    _close(feat.detach(), f1, 1e-10)
    _close_grads({k: v.grad for k, v in m.named_parameters()}, g1, 1e-9)

    # CLIP ViT: dropout on the attention probabilities only
    wv = {k: v.double() for k, v in E.seeded_weights(E.vit_shapes(layers=layers), 65).items()}
    frames = E.synthetic_frames(66, 2, 1).double()
    vm = R.vision_masks(12, 5, 2, 50, layers, p_attn=p)
    cfgv = transformers.CLIPVisionConfig(num_hidden_layers=layers, attention_dropout=p, attn_implementation="eager")
    mv = transformers.CLIPVisionModelWithProjection(cfgv).double()
    mv.load_state_dict(wv, strict=True)
    mv.train()
    q = _MaskQueue([vm[("attn", i)] for i in range(layers)], p)
    monkeypatch.setattr(torch.nn.functional, "dropout", q)
    e = mv(pixel_values=frames[:, 0]).image_embeds
    e = e / (e.norm(dim=-1, keepdim=True) + 1e-9)
    E.probe_loss(e, 10).backward()
    monkeypatch.undo()
    assert q.calls == layers
    f1, g1 = R.visual_feature_grads(wv, frames, 10, masks=vm)
    # (CLIP's eager attention takes its softmax in float32 whatever the model's dtype: ~3e-8 relative here; a wrong or misplaced
    # mask moves the result by ~1e-1)
    _close(e.detach(), f1, 1e-6)
    _close_grads({k: v.grad for k, v in mv.named_parameters()}, g1, 1e-5)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.999])
def test_dropout_probabilities_in_range_are_accepted(p):
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.trainer import TrainConfig
    t = BertTextEncoder(layers=1, vocab_size=50, hidden_dropout_prob=p, attention_probs_dropout_prob=p)
    v = ClipVisualEncoder(layers=1, attention_dropout=p)
    assert t.hidden_dropout_prob == t.attention_probs_dropout_prob == v.attention_dropout == p
    assert TrainConfig(data_root="", ocr_phrase_pkl=None, train_encoders=True, encoder_dropout=p).encoder_dropout == p


def test_defaults_are_no_dropout():
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.trainer import TrainConfig
    t, v = BertTextEncoder(layers=1, vocab_size=50), ClipVisualEncoder(layers=1)
    assert t.hidden_dropout_prob == t.attention_probs_dropout_prob == v.attention_dropout == 0.0
    assert TrainConfig(data_root="", ocr_phrase_pkl=None).encoder_dropout is None


@pytest.mark.parametrize("p", [1.0, -0.1])
def test_dropout_probabilities_out_of_range_are_refused_by_name(p):
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.trainer import TrainConfig
    for name in ("hidden_dropout_prob", "attention_probs_dropout_prob"):
        with pytest.raises(ValueError, match=name):
            BertTextEncoder(layers=1, vocab_size=50, **{name: p})
    with pytest.raises(ValueError, match="attention_dropout"):
        ClipVisualEncoder(layers=1, attention_dropout=p)
    with pytest.raises(ValueError, match="encoder_dropout"):
        TrainConfig(data_root="", ocr_phrase_pkl=None, train_encoders=True, encoder_dropout=p)


def test_encoder_dropout_overrides_all_three_probabilities():
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.trainer import TrainConfig, apply_encoder_dropout
    t = BertTextEncoder(layers=1, vocab_size=50, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2)
    v = ClipVisualEncoder(layers=1, attention_dropout=0.4)
    apply_encoder_dropout(TrainConfig(data_root="", ocr_phrase_pkl=None, train_encoders=True), t, v)      # None: the encoders' own
    assert (t.hidden_dropout_prob, t.attention_probs_dropout_prob, v.attention_dropout) == (0.3, 0.2, 0.4)
    apply_encoder_dropout(TrainConfig(data_root="", ocr_phrase_pkl=None, train_encoders=False, encoder_dropout=0.1), t, v)    # frozen: unused
    assert (t.hidden_dropout_prob, t.attention_probs_dropout_prob, v.attention_dropout) == (0.3, 0.2, 0.4)
    apply_encoder_dropout(TrainConfig(data_root="", ocr_phrase_pkl=None, train_encoders=True, encoder_dropout=0.1), t, v)
    assert t.hidden_dropout_prob == t.attention_probs_dropout_prob == v.attention_dropout == 0.1
