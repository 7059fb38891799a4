"""GPU: train-mode dropout of the trainable encoders (BertTextEncoder.hidden_dropout_prob / .attention_probs_dropout_prob,
ClipVisualEncoder.attention_dropout, TrainConfig.encoder_dropout) against the float64 restatement tests/encoder_dropout_ref.py,
whose masks come from tests/dropout_mirror.py with the kernels' element numbering and tags -- pinned on the CPU to HF's own
train-mode models (tests/test_encoder_dropout_ref.py).  p = 0.1 at every site.

Bounds are those of the corresponding p = 0 tests of tests/test_gpu_encoder_train.py.  Negative controls rerun the restatement
with wrong masks (the next step's; the attention masks transposed; the attn-out and ffn-out masks swapped): each must miss the
relative-L2 gradient bound by at least 10x, so a bound that passes is evidence of the right masks at the right sites, not of loose
tolerances.  (The controls are measured on the tensors whose gradient is at least 1 % of the largest one's, without _compare's
absolute floor: that floor exists for the key biases, whose gradient is zero up to rounding, and it is large enough to hide a
transposed attention mask -- which moves the q / k weight gradients by ~25 % relative at p = 0.1.)"""
import pytest
import torch

from tests import encoder_dropout_ref as R
from tests.test_gpu_encoder_train import BERT12_LAYER_BOUNDS, _compare, _per_layer, _standalone

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 0.1


def _miss(arena, ref, rel_bound):
    """The largest relative-L2 gradient error / rel_bound over the tensors whose gradient norm is >= 1 % of the largest one's."""
    top = max(r.norm().item() for r in ref.values())
    return max((arena.grad_view(k).cpu().double() - r.double()).norm().item() / (rel_bound * r.norm().item())
               for k, r in ref.items() if r.norm().item() >= 1e-2 * top)


def _text(layers, B, Lq, one_token_row=False, p_hidden=P, p_attn=P):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoder_train import TextBackprop
    from ultrafnd_git_amd.encoders import BertTextEncoder
    w = E.seeded_weights(E.bert_shapes(layers=layers, vocab=1000), 40 + Lq)
    ids, mask = E.synthetic_tokens(400 + Lq, B, Lq, vocab=1000)
    if one_token_row:
        mask[1] = 0
        mask[1, 0] = 1
    enc = BertTextEncoder(layers=layers, vocab_size=1000, hidden_dropout_prob=p_hidden, attention_probs_dropout_prob=p_attn)
    enc.load_state_dict(w)
    bp, arena = _standalone(TextBackprop, enc.to(DEV))
    return w, ids, mask, bp, arena


def _state(bp):
    st = bp.rng().read()
    return int(st.seed), int(st.step)


@pytest.mark.parametrize("B,Lq,one_token_row", [(4, 64, False), (4, 128, False), (3, 77, True), (8, 256, False)])
def test_text_encoder_dropout_vs_float64_restatement(B, Lq, one_token_row):
    w, ids, mask, bp, arena = _text(2, B, Lq, one_token_row)
    feat = bp.forward_train(ids, mask).clone()
    seed, step = _state(bp)
    assert step == 1                   # the encoder's own state: advanced by the forward
    masks = R.text_masks(seed, step, B, Lq, 2, p_hidden=P, p_attn=P)
    ref_feat, ref = R.text_feature_grads(w, ids, mask, 78, masks=masks)
    assert (feat.cpu().double() - ref_feat).abs().max().item() <= 1.2e-3
    dfeat = torch.randn(ref_feat.shape, generator=torch.Generator().manual_seed(78)).to(DEV)
    bp.backward(dfeat)
    torch.cuda.synchronize()
    _compare(arena, ref, 1.6e-2, f"dropout 0.1, B={B} L={Lq} (2 layers)")
    if (B, Lq) != (4, 64):
        return
    # negative controls: each misses the bound by >= 10x
    ok = _miss(arena, ref, 1.6e-2)
    controls = {"step + 1": R.text_masks(seed, step + 1, B, Lq, 2, p_hidden=P, p_attn=P)}
    tr = dict(masks)
    for i in range(2):
        tr[("attn", i)] = masks[("attn", i)].transpose(-1, -2).contiguous()
    controls["attention q <-> k"] = tr
    sw = dict(masks)
    for i in range(2):
        sw[("attn_out", i)], sw[("ffn_out", i)] = masks[("ffn_out", i)], masks[("attn_out", i)]
    controls["attn-out <-> ffn-out"] = sw
    for name, m in controls.items():
        _, bad = R.text_feature_grads(w, ids, mask, 78, masks=m)
        miss = _miss(arena, bad, 1.6e-2)
        print(f"negative control {name}: {miss:.1f} x the bound (the right masks: {ok:.2f} x)")
        assert miss >= 10.0 and miss >= 10.0 * ok, (name, miss, ok)


@pytest.mark.parametrize("B,Fr", [(2, 1), (3, 3)])
def test_visual_encoder_dropout_vs_float64_restatement(B, Fr):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoder_train import VisualBackprop
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    w = E.seeded_weights(E.vit_shapes(layers=2), 50 + Fr)
    frames = E.synthetic_frames(500 + Fr, B, Fr)
    enc = ClipVisualEncoder(layers=2, attention_dropout=P)
    enc.load_state_dict(w)
    bp, arena = _standalone(VisualBackprop, enc.to(DEV))
    feat = bp.forward_train(frames).clone()
    seed, step = _state(bp)
    masks = R.vision_masks(seed, step, B * Fr, enc.n_patches + 1, 2, p_attn=P)
    ref_feat, ref = R.visual_feature_grads(w, frames, 79, masks=masks)
    assert (feat.cpu().double() - ref_feat).abs().max().item() <= 1.5e-3
    bp.backward(torch.randn(ref_feat.shape, generator=torch.Generator().manual_seed(79)).to(DEV))
    torch.cuda.synchronize()
    _compare(arena, ref, 1.6e-2, f"ViT dropout 0.1, B={B} F={Fr} (2 layers)")
    ok = _miss(arena, ref, 1.6e-2)
    _, bad = R.visual_feature_grads(w, frames, 79, masks=R.vision_masks(seed, step + 1, B * Fr, enc.n_patches + 1, 2, p_attn=P))
    miss = _miss(arena, bad, 1.6e-2)
    tr = {k: v.transpose(-1, -2).contiguous() for k, v in masks.items()}
    _, bad_t = R.visual_feature_grads(w, frames, 79, masks=tr)
    miss_t = _miss(arena, bad_t, 1.6e-2)
    print(f"ViT negative controls: step + 1 {miss:.1f} x, q <-> k {miss_t:.1f} x the bound (the right masks: {ok:.2f} x)")
    assert min(miss, miss_t) >= 10.0 and min(miss, miss_t) >= 10.0 * ok, (miss, miss_t, ok)


def test_full_depth_text_encoder_dropout_sampled_tensors():
    w, ids, mask, bp, arena = _text(12, 4, 128)
    bp.forward_train(ids, mask)
    seed, step = _state(bp)
    masks = R.text_masks(seed, step, 4, 128, 12, p_hidden=P, p_attn=P)
    _, ref = R.text_feature_grads(w, ids, mask, 5, masks=masks, dtype=torch.float32)
    bp.backward(torch.randn(4, 768, generator=torch.Generator().manual_seed(5)).to(DEV))
    torch.cuda.synchronize()
    keep = {k: v for k, v in ref.items() if k.startswith(("encoder.layer.0.", "encoder.layer.6.", "encoder.layer.11.", "embeddings."))}
    _compare(arena, keep, 3.0e-2, "BERT 12 layers, dropout 0.1, sampled tensors")
    per = _per_layer(arena, ref, "encoder.layer.{}.", (0, 6, 11))
    print("BERT 12 layers, dropout 0.1, per-layer relative L2:", {k: f"{v:.3e}" for k, v in per.items()})
    assert per[11] <= BERT12_LAYER_BOUNDS[11] and per[6] <= BERT12_LAYER_BOUNDS[6] and per[0] <= BERT12_LAYER_BOUNDS[0], per


def test_explicit_zero_is_bit_identical_to_the_default():
    """p = 0 runs the launches it ran before dropout existed: same bits as an encoder built without the arguments, and the
    encoder's own step state is never touched."""
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoder_train import TextBackprop, VisualBackprop
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    w = E.seeded_weights(E.bert_shapes(layers=2, vocab=1000), 41)
    ids, mask = E.synthetic_tokens(401, 3, 77, vocab=1000)
    dfeat = torch.randn(3, 768, generator=torch.Generator().manual_seed(3)).to(DEV)
    grads = []
    for kw in ({}, {"hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0}):
        enc = BertTextEncoder(layers=2, vocab_size=1000, **kw)
        enc.load_state_dict(w)
        bp, arena = _standalone(TextBackprop, enc.to(DEV))
        f = bp.forward_train(ids, mask).clone()
        bp.backward(dfeat)
        torch.cuda.synchronize()
        assert bp.drop_state is None
        grads.append((f, torch.nan_to_num(arena.grad, nan=-7.0).clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    wv = E.seeded_weights(E.vit_shapes(layers=1), 42)
    frames = E.synthetic_frames(402, 2, 1)
    out = []
    for kw in ({}, {"attention_dropout": 0.0}):
        enc = ClipVisualEncoder(layers=1, **kw)
        enc.load_state_dict(wv)
        bp, arena = _standalone(VisualBackprop, enc.to(DEV))
        f = bp.forward_train(frames).clone()
        bp.backward(torch.ones(2, 512, device=DEV))
        torch.cuda.synchronize()
        out.append((f, torch.nan_to_num(arena.grad, nan=-7.0).clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_frozen_forward_never_drops():
    """forward() of an encoder built with p = 0.1 (train or eval mode) equals the p = 0 encoder's bit for bit."""
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    w = E.seeded_weights(E.bert_shapes(layers=2, vocab=1000), 43)
    ids, mask = E.synthetic_tokens(403, 4, 128, vocab=1000)
    encs = [BertTextEncoder(layers=2, vocab_size=1000, hidden_dropout_prob=p, attention_probs_dropout_prob=p) for p in (0.0, P)]
    for e in encs:
        e.load_state_dict(w)
    encs = [e.to(DEV) for e in encs]
    encs[1].train()
    a, b = encs[0](ids.to(DEV), mask.to(DEV)), encs[1](ids.to(DEV), mask.to(DEV))
    assert torch.equal(a, b)
    wv = E.seeded_weights(E.vit_shapes(layers=2), 44)
    frames = E.synthetic_frames(404, 2, 1).to(DEV)
    vencs = [ClipVisualEncoder(layers=2, attention_dropout=p) for p in (0.0, P)]
    for e in vencs:
        e.load_state_dict(wv)
    vencs = [e.to(DEV) for e in vencs]
    vencs[1].train()
    assert torch.equal(vencs[0](frames), vencs[1](frames))


# ------------------------------------------------------------------ the trainer
def _trainer(tmp_path, name, encoder_dropout, seed_offset=0):
    from oracle import encoders_ref as E
    from oracle import tier_a as O
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    B = 4
    wt = E.seeded_weights(E.bert_shapes(layers=2, vocab=500), 11)
    wv = E.seeded_weights(E.vit_shapes(layers=2), 12)
    tenc, venc = BertTextEncoder(layers=2, vocab_size=500), ClipVisualEncoder(layers=2)
    tenc.load_state_dict(wt); venc.load_state_dict(wv)
    fus_sd, clf_sd = O.seeded_params(1234)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path / name), batch_size=B, device=DEV, use_graph=False, encode_inline=True,
                      train_encoders=True, grad_clip=1e9, encoder_dropout=encoder_dropout)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(16, seed=1), text_encoder=tenc.to(DEV), visual_encoder=venc.to(DEV))
    tr.fusion.load_state_dict(fus_sd); tr.clf.load_state_dict(clf_sd)
    tr.fusion.dropout = tr.clf.dropout = tr.clf.node_dropout = 0.0
    tr.head.step_bufs.clear()
    tr.fusion.train(); tr.clf.train()
    return tr, wt, wv, fus_sd, clf_sd


def _batch(step=0):
    from oracle import encoders_ref as E
    from oracle import tier_a as O
    B, Lq = 4, 64
    ids, mask = E.synthetic_tokens(13 + 10 * step, B, Lq, vocab=500, min_len=8)
    frames = E.synthetic_frames(14 + 10 * step, B, 1)
    batch = O.seeded_batch(15 + 10 * step, B)
    gb = {k: v.to(DEV) for k, v in batch.items()}
    gb.update({"input_ids": ids.to(DEV), "attention_mask": mask.to(torch.int32).to(DEV), "frames": frames.to(DEV)})
    return batch, ids, mask, frames, gb


def test_trainer_step_with_encoder_dropout_vs_oracle(tmp_path):
    """ForensicTrainer(train_encoders=True, encoder_dropout=0.1): one step against the restatement (masks of the head's step
    state: seed, step 0) + oracle.tier_a -- loss, global gradient norm, every encoder gradient -- as
    test_trainer_step_with_trainable_encoders_vs_oracle does with dropout off."""
    import torch.nn.functional as F
    from oracle import tier_a as O
    tr, wt, wv, fus_sd, clf_sd = _trainer(tmp_path, "a", P)
    assert tr.text_encoder.hidden_dropout_prob == tr.text_encoder.attention_probs_dropout_prob == tr.visual_encoder.attention_dropout == P
    assert tr.text_bp.rng() is tr.optim.state and tr.vis_bp.rng() is tr.optim.state
    batch, ids, mask, frames, gb = _batch()
    st0 = tr.optim.state.read()
    seed, step = int(st0.seed), int(st0.step)
    tr.train_step(gb)
    st = tr.optim.state.read()
    assert int(st.step) == step + 1
    tm = R.text_masks(seed, step, 4, 64, 2, p_hidden=P, p_attn=P)
    vm = R.vision_masks(seed, step, 4, 50, 2, p_attn=P)
    wtl = {k: v.clone().requires_grad_(True) for k, v in wt.items()}
    wvl = {k: v.clone().requires_grad_(True) for k, v in wv.items()}
    fl = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in fus_sd.items()}
    cl = {k: v.clone().requires_grad_(v.is_floating_point() and not k.endswith("tau")) for k, v in clf_sd.items()}
    rb = dict(batch)
    rb["text_features"], rb["visual_features"] = R.text_features(wtl, ids, mask, masks=tm), R.visual_features(wvl, frames, masks=vm)
    ro = O.forward_batch(fl, cl, rb)
    loss = F.cross_entropy(ro["logits"], batch["label"])
    loss.backward()
    assert abs(float(st.loss) - float(loss)) <= 1e-3
    grads = {"text." + k: v.grad for k, v in wtl.items() if v.grad is not None}
    grads.update({"vis." + k: v.grad for k, v in wvl.items() if v.grad is not None})
    enc_norm = sum(float(g.double().pow(2).sum()) for g in grads.values()) ** 0.5
    head_norm = sum(float(v.grad.double().pow(2).sum()) for d in (fl, cl) for v in d.values() if v.requires_grad and v.grad is not None) ** 0.5
    total = (enc_norm ** 2 + head_norm ** 2) ** 0.5
    print(f"dropout 0.1: loss {float(st.loss):.6f} (oracle {float(loss):.6f}); grad norm {float(st.grad_norm):.5f} (oracle {total:.5f}), "
          f"relative error {abs(float(st.grad_norm) - total) / total:.3e}")
    assert abs(float(st.grad_norm) - total) <= 1e-5 * total
    _compare(tr.arena, grads, 2.5e-2, "trainer step with encoder dropout 0.1, encoder gradients")


def test_trainer_validation_features_never_drop_and_runs_are_reproducible(tmp_path):
    """Before any step, val and test features of a trainer with encoder_dropout=0.1 equal those of one without, bit for bit.  Two
    trainers from one seed then run 3 steps with dropout and end with bit-identical arenas (masters and gradients); and
    encoder_dropout=0.0 is bit-identical to None over a step."""
    a = _trainer(tmp_path, "a", P)[0]
    b = _trainer(tmp_path, "b", P)[0]
    z = _trainer(tmp_path, "z", None)[0]
    _, _, _, _, gb = _batch()
    for split in ("val", "test"):
        fa, fz = a.head.bufs(4, False), z.head.bufs(4, False)
        a._load_batch(fa, gb, split)
        ta, va = fa["text"].clone(), fa["visual"].clone()
        z._load_batch(fz, gb, split)
        torch.cuda.synchronize()
        assert torch.equal(ta, fz["text"]) and torch.equal(va, fz["visual"]), split
    for s in range(3):
        gb = _batch(s)[4]
        a.train_step(gb)
        b.train_step(gb)
    torch.cuda.synchronize()
    assert torch.equal(a.arena.data, b.arena.data)
    assert torch.equal(torch.nan_to_num(a.arena.grad, nan=-7.0), torch.nan_to_num(b.arena.grad, nan=-7.0))
    z0 = _trainer(tmp_path, "z0", 0.0)[0]
    gb = _batch()[4]
    z.train_step(gb)
    z0.train_step(gb)
    torch.cuda.synchronize()
    assert torch.equal(z.arena.data, z0.arena.data)
