"""GPU: gradient accumulation over micro-batches -- ufnd_grad_accumulate, the `micro` word of the dropout key, and the trainer's
k-micro-batch optimizer step (head only and with trainable encoders) against the references of the single-batch step.

Convention under test: batch_size is the micro-batch, grad_accum_steps = k, the gradient applied is (1 / k) sum_j grad(mean CE of
micro-batch j); arena.grad holds the SUM, state.grad_scale the 1 / k.  Equal micro-batches make that the full-batch gradient, so the
fixtures and oracles of the k = 1 tests apply with their own bounds."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import dropout_mirror as D
from tests.helpers import assert_digest_close, load_npz, nograd_keys

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = 1         # UFND_ERR_INVALID


def _L():
    from ultrafnd_git_amd import _lib as L
    return L


def _accumulate(dst, src, n, overwrite, state=None):
    L = _L()
    return L.lib().ufnd_grad_accumulate(dst.data_ptr(), src.data_ptr(), n, int(overwrite), None if state is None else state.ptr,
                                        L.stream_ptr(dst.device))


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("n", [4, 1020, 4 * (2 * 1024 * 256 + 1)], ids=["one-vector", "partial-block", "past-one-sweep"])
def test_accumulate_kernel_is_torch_add_and_a_bit_copy(n):
    """dst += src is torch.add bit for bit, the overwrite form copies the bits (NaN payloads, -0.0, denormals included); the four
    guard floats either side of the range stay as they were, src is unchanged."""
    g = torch.Generator().manual_seed(n)
    G = 4                                                   # guard floats (keeps the range 16-byte aligned)
    src_all = torch.randn(n + 2 * G, generator=g).to(DEV)
    dst_all = (torch.randn(n + 2 * G, generator=g) * 3.0).to(DEV)
    special = torch.tensor([float("nan"), -0.0, 1e-41, float("inf")])[: min(4, n)]
    src_all[G:G + special.numel()] = special.to(DEV)
    src0, dst0 = src_all.clone(), dst_all.clone()
    src, dst = src_all[G:G + n], dst_all[G:G + n]
    assert _accumulate(dst, src, n, False) == 0
    torch.cuda.synchronize()
    want = torch.add(dst0[G:G + n], src0[G:G + n])
    assert torch.equal(dst.view(torch.int32), want.view(torch.int32))
    assert torch.equal(dst_all[:G], dst0[:G]) and torch.equal(dst_all[G + n:], dst0[G + n:])
    assert torch.equal(src_all.view(torch.int32), src0.view(torch.int32))
    assert _accumulate(dst, src, n, True) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int32), src0[G:G + n].view(torch.int32))
    assert torch.equal(dst_all[:G], dst0[:G]) and torch.equal(dst_all[G + n:], dst0[G + n:])
    assert torch.equal(src_all.view(torch.int32), src0.view(torch.int32))


def test_accumulate_counts_micro_batches_and_every_step_advance_clears_the_count():
    from ultrafnd_git_amd.state import StepStateBuffer
    L = _L()
    dev = torch.device(DEV, torch.cuda.current_device())
    st = StepStateBuffer(dev, seed=3)
    n = 1024
    p, g, m, v, acc = (torch.randn(n, device=dev) for _ in range(5))
    m.zero_(); v.abs_()
    partials = torch.empty(1024, device=dev)
    assert st.read().micro == 0
    assert _accumulate(acc, g, n, True) == 0                 # NULL state: not counted
    assert st.read().micro == 0
    assert _accumulate(acc, g, n, True, st) == 0
    assert st.read().micro == 1
    assert _accumulate(acc, g, n, False, st) == 0
    s = st.read()
    assert s.micro == 2 and s.step == 0
    L.check(L.lib().ufnd_clip_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, partials.data_ptr(), st.ptr,
                                         L.stream_ptr(dev)), "ufnd_clip_adamw_step")
    s = st.read()
    assert s.micro == 0 and s.step == 1
    assert _accumulate(acc, g, n, False, st) == 0
    assert st.read().micro == 1
    st.advance()                                             # ufnd_step_advance
    s = st.read()
    assert s.micro == 0 and s.step == 2
    assert list(s.reserved) == [0.0, 0.0]


def test_accumulate_rejects_bad_arguments():
    L = _L()
    a, b = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    s = L.stream_ptr(a.device)
    fn = L.lib().ufnd_grad_accumulate
    assert fn(a.data_ptr(), b.data_ptr(), 6, 0, None, s) == INVALID               # n % 4
    assert fn(a.data_ptr() + 4, b.data_ptr(), 8, 0, None, s) == INVALID           # dst 4 bytes off the 16-byte grid
    assert fn(a.data_ptr(), b.data_ptr() + 4, 8, 0, None, s) == INVALID
    assert fn(None, b.data_ptr(), 8, 0, None, s) == INVALID
    assert fn(a.data_ptr(), None, 8, 0, None, s) == INVALID
    assert fn(a.data_ptr(), a.data_ptr() + 16, 8, 0, None, s) == INVALID          # overlapping ranges
    torch.cuda.synchronize()
    assert not a.any() and not b.any()


# ---------------------------------------------------------------------------------------------------------------- trainer helpers
def _trainer(tmp_path, B, use_graph=True, n=64, seed_params=None, dropout_off=False, **kw):
    from oracle import tier_a as O
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=B, device=DEV, use_graph=use_graph, **kw)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(n, seed=3))
    if seed_params is not None:
        fus_sd, clf_sd = O.seeded_params(seed_params)
        tr.fusion.load_state_dict(fus_sd)
        tr.clf.load_state_dict(clf_sd)
    if dropout_off:
        tr.fusion.dropout = tr.clf.dropout = tr.clf.node_dropout = 0.0
    tr.fusion.train(); tr.clf.train()
    return tr


def _golden_batch(z):
    return {k: torch.from_numpy(z[f"in/{k}"]).to(DEV) for k in
            ("text_features", "audio_features", "visual_features", "temporal_features", "gnn_feat", "aux", "label")}


def _rows(batch, lo, hi):
    return {k: v[lo:hi].contiguous() for k, v in batch.items()}


# ---------------------------------------------------------------------------------------------------------------- 2. reference parity
@pytest.mark.parametrize("use_graph", [False, True])
def test_four_micro_batches_of_eight_match_the_reference_step_of_32(tmp_path, use_graph):
    """The B = 32 golden batch as four row slices of 8 with grad_accum_steps = 4, three optimizer steps == the reference's three
    steps on the 32 rows, at the bounds of tests/test_gpu_trainer.py::test_fused_step_matches_reference (loss 5e-5, logits 1e-4,
    parameters rtol 2e-5 / atol 2e-7) and of tests/test_gpu_tier_a.py (gradients 2e-4, norm 1e-3 against the reference's fp32 norm)."""
    z = load_npz("tier_a_B32.npz")
    tr = _trainer(tmp_path, 8, use_graph, seed_params=int(z["param_seed"]), dropout_off=True, grad_accum_steps=4)
    batch = _golden_batch(z)
    for step in (1, 2, 3):
        losses, logits = [], []
        for j in range(4):
            out = tr.train_step(_rows(batch, 8 * j, 8 * j + 8))
            losses.append(float(out["loss"].cpu()))
            logits.append(out["logits"].cpu().numpy().copy())
            assert tr.optim.pending == (j + 1) % 4
        st = tr.optim.state.read()
        assert int(st.step) == step and st.micro == 0
        loss = sum(losses) / 4
        lerr = np.abs(np.concatenate(logits) - z[f"step{step}/logits"]).max()
        print(f"graph={use_graph} step {step}: mean micro-loss {loss:.7f} (ref {float(z[f'step{step}/loss']):.7f}), logits max-abs-err {lerr:.2e}, "
              f"grad norm {st.grad_norm:.6f} (ref {float(z[f'step{step}/grad_norm']):.6f})")
        assert abs(loss - float(z[f"step{step}/loss"])) <= 5e-5, (step, loss)
        assert lerr <= 1e-4, (step, lerr)
        if step == 1:
            assert st.grad_scale == 0.25
            ref_norm = float(z["step1/grad_norm"])
            assert abs(st.grad_norm - ref_norm) <= 1e-3 * ref_norm, (st.grad_norm, ref_norm)
            bad = []
            nograd = set(nograd_keys(z))
            for pre, mod in (("fusion.", tr.fusion), ("clf.", tr.clf)):
                for k, _ in mod.named_parameters():
                    if not tr.arena.has_grad(mod.akey(k)):
                        assert pre + k in nograd, k
                        continue
                    assert pre + k not in nograd, k
                    try:
                        assert_digest_close(z, f"grad/{pre}{k}", mod.gview(k).detach() * st.grad_scale, rtol=2e-4, atol=1e-8)
                    except AssertionError as e:
                        bad.append(str(e)[:300])
            assert not bad, "\n".join(bad)
    assert int(tr.optim.state.read().step) == 3
    for k, p in list(("fusion." + k, p) for k, p in tr.fusion.named_parameters()) + \
            list(("clf." + k, p) for k, p in tr.clf.named_parameters()):
        if p.dim():
            assert_digest_close(z, f"param_step3/{k}", p.detach(), rtol=2e-5, atol=2e-7)


# ---------------------------------------------------------------------------------------------------------------- 3. off means off
def test_one_micro_batch_per_step_is_the_step_without_the_option(tmp_path):
    res = []
    for kw in ({}, {"grad_accum_steps": 1}):
        torch.manual_seed(5)
        tr = _trainer(tmp_path, 16, True, **kw)
        assert tr.fusion.dropout > 0 and tr.clf.dropout > 0
        it = iter(tr.train_loader)
        for _ in range(3):
            out = tr.train_step(next(it))
            assert tr.optim.state.read().micro == 0 and tr.optim.pending == 0
        assert tr.arena.grad_acc is None and tr.optim.accum_steps == 1
        assert not tr.reducer.hold and tr.reducer.before_bucket is None
        assert tr.flush_accumulated() is False
        st = tr.optim.state.read()
        assert int(st.step) == 3 and st.grad_scale == 1.0
        res.append((out["logits"].clone(), tr.arena.data.clone(), float(st.grad_norm)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


# ---------------------------------------------------------------------------------------------------------------- 4. masks
def test_masks_differ_per_micro_batch_repeat_per_run_and_follow_the_mirror(tmp_path):
    """Dropout on, k = 2, the SAME 8 rows as both micro-batches (the parameters do not move between them): the two forwards differ
    only by their masks.  Micro-batch 0 draws the mirror's masks at (seed, step), micro-batch 1 at (seed, step + (1 << 40)): the
    float64 oracle with those masks gives each micro-batch's logits within tests/test_gpu_head_geometry.py's 2e-5, and with the other
    micro-batch's masks (or the next step's) misses it by 10 x at least."""
    from oracle import tier_a as O
    z = load_npz("tier_a_B32.npz")
    batch = _rows(_golden_batch(z), 0, 8)
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        tr = _trainer(tmp_path, 8, True, seed_params=int(z["param_seed"]), grad_accum_steps=2)
        st0 = tr.optim.state.read()
        assert st0.micro == 0 and st0.step == 0
        l0 = tr.train_step(batch)["logits"].clone()
        st1 = tr.optim.state.read()
        assert st1.micro == 1 and st1.step == 0 and tr.optim.pending == 1
        l1 = tr.train_step(batch)["logits"].clone()
        st2 = tr.optim.state.read()
        assert st2.micro == 0 and st2.step == 1 and tr.optim.pending == 0
        runs.append((l0, l1, tr.arena.data.clone()))
    assert not torch.equal(runs[0][0], runs[0][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    # the mirror
    fus_sd, clf_sd = O.seeded_params(int(z["param_seed"]))
    f64 = [{k: v.double() for k, v in d.items()} for d in (fus_sd, clf_sd)]
    cb = {k: v.cpu() for k, v in batch.items()}
    H, T = tr.fusion.hidden, tr.clf.node_trees
    ps = (tr.fusion.dropout, tr.clf.dropout, tr.clf.node_dropout)
    assert min(ps) > 0
    seed = int(st0.seed)

    def oracle(step_key):
        masks = D.head_masks(8, H, T, *ps, (seed, step_key))
        return O.forward_batch(*f64, cb, train=True, masks=masks)["logits"].detach()
    refs = {"micro 0": oracle(0), "micro 1": oracle(1 << 40), "step 1": oracle(1)}
    TOL, WIDE = 2e-5, 10.0
    for name, got, own in (("micro-batch 0", runs[0][0], "micro 0"), ("micro-batch 1", runs[0][1], "micro 1")):
        errs = {k: (got.double().cpu() - r).abs().max().item() for k, r in refs.items()}
        print(f"{name}: logits max-abs-err against the oracle with the masks of " + ", ".join(f"{k}: {e:.2e}" for k, e in errs.items()))
        assert errs[own] <= TOL, (name, errs)
        assert all(e >= WIDE * TOL for k, e in errs.items() if k != own), (name, errs)


# ---------------------------------------------------------------------------------------------------------------- 5. flush
def test_flush_after_three_of_four_equals_a_group_of_three(tmp_path):
    """k = 4, three micro-batches, flush_accumulated() == k = 3 fed the same three: the first sums (g1 + g2) + g3 in the accumulator
    and loads it, the second folds (g1 + g2) into g3 -- fp32 addition commutes, both divide by 3 -- so the bits agree."""
    res = []
    for k, flush in ((4, True), (3, False)):
        torch.manual_seed(5)
        tr = _trainer(tmp_path, 8, True, grad_accum_steps=k)
        it = iter(tr.train_loader)
        for _ in range(3):
            out = tr.train_step(next(it))
        logits = out["logits"].clone()
        if flush:
            assert tr.optim.pending == 3 and int(tr.optim.state.read().step) == 0
            assert tr.flush_accumulated() is True
        st = tr.optim.state.read()
        assert int(st.step) == 1 and st.micro == 0 and tr.optim.pending == 0
        assert st.grad_scale == np.float32(1.0 / 3.0)
        res.append((logits, tr.arena.data.clone(), tr.arena.grad.clone(), float(st.grad_norm)))
        if flush:
            assert tr.flush_accumulated() is False
            torch.cuda.synchronize()
            assert torch.equal(tr.arena.data, res[-1][1]) and int(tr.optim.state.read().step) == 1
    assert all(torch.equal(a, b) for a, b in zip(res[0][:3], res[1][:3])) and res[0][3] == res[1][3]


# ---------------------------------------------------------------------------------------------------------------- 6. epoch loop
def test_fit_steps_once_per_group_and_flushes_the_short_last_group(tmp_path, capsys):
    """A train split of 35 rows in batches of 8 is 5 micro-batches; with k = 2 one epoch takes 2 + 2 + 1 -> three optimizer steps."""
    import re
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=8, epochs=1, device=DEV, grad_accum_steps=2)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(50, seed=3))
    assert [int(b["label"].shape[0]) for b in tr.train_loader] == [8, 8, 8, 8, 3]
    tr.train_loader.epoch = 0
    tr.fit()
    st = tr.optim.state.read()
    assert int(st.step) == 3 and st.micro == 0 and tr.optim.pending == 0
    assert st.grad_scale == 1.0                               # the flushed group had one micro-batch
    out = capsys.readouterr().out
    print(out[-600:])
    loss = float(re.search(r"train_loss=([0-9.eE+-]+|nan|inf)", out).group(1))
    assert math.isfinite(loss) and 0.0 < loss < 5.0
    assert torch.isfinite(tr.arena.data).all()


def test_pipelined_steps_refuse_accumulation(tmp_path):
    tr = _trainer(tmp_path, 8, True, grad_accum_steps=2)
    for call in (lambda: tr.train_step_pipelined({}, None), lambda: tr.train_group_pipelined({}, None)):
        with pytest.raises(ValueError, match="grad_accum_steps=2"):
            call()


# ---------------------------------------------------------------------------------------------------------------- 7. trainable encoders
# tests/test_gpu_encoder_train.py's criterion for every encoder gradient tensor: relative L2 <= 2.5e-2 of the oracle's, plus an
# absolute floor of 2e-3 x the largest per-element gradient scale x sqrt(numel) for tensors whose own gradient is (nearly) zero.
ENC_GRAD_REL = 2.5e-2
# global gradient norm against the oracle's float64 total: 2 x measured on MI355X, as that file sets its own (1e-5 = 2 x 4.7e-6 for
# the single batch of four rows).  Measured for 2 x 2 rows accumulated: 4.75e-6 (norm 2.68139 against the oracle's 2.68138).
ACCUM_NORM_REL = 9.5e-6


def _compare(arena, scale, ref, rel_bound, what):
    top = max(g.norm().item() / max(1, g.numel()) ** 0.5 for g in ref.values())
    worst = ("", 0.0)
    for k, r in ref.items():
        got = arena.grad_view(k).cpu() * scale
        assert torch.isfinite(got).all(), (what, k)
        err = (got - r).norm().item()
        rel = err / max(r.norm().item(), 1e-30)
        floor = 2e-3 * top * max(1, r.numel()) ** 0.5
        if err > floor and rel > worst[1]:
            worst = (k, rel)
        assert err <= rel_bound * r.norm().item() + floor, (what, k, rel, err, floor)
    print(f"{what}: worst relative-L2 gradient error {worst[1]:.3e} ({worst[0]}), bound {rel_bound:.1e}")


def test_trainable_encoders_two_micro_batches_of_two_vs_autograd_over_four_rows(tmp_path):
    """ForensicTrainer(train_encoders=True, batch_size=2, grad_accum_steps=2) on the four rows of
    test_trainer_step_with_trainable_encoders_vs_oracle (2 + 2 layers, L = 64, grad_clip 1e9, dropout 0) as two micro-batches of
    two rows, against autograd over all four: mean micro-loss, the global norm, every encoder gradient tensor; the encoders' bf16
    operands were refreshed once -- by the optimizer step, not by the accumulating micro-batch."""
    import torch.nn.functional as F
    from oracle import encoders_ref as E
    from oracle import tier_a as O
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    B, Lq = 4, 64
    wt = E.seeded_weights(E.bert_shapes(layers=2, vocab=500), 11)
    wv = E.seeded_weights(E.vit_shapes(layers=2), 12)
    tenc, venc = BertTextEncoder(layers=2, vocab_size=500), ClipVisualEncoder(layers=2)
    tenc.load_state_dict(wt); venc.load_state_dict(wv)
    tenc, venc = tenc.to(DEV), venc.to(DEV)
    ids, mask = E.synthetic_tokens(13, B, Lq, vocab=500, min_len=8)
    frames = E.synthetic_frames(14, B, 1)
    batch = O.seeded_batch(15, B)
    fus_sd, clf_sd = O.seeded_params(1234)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=2, device=DEV, use_graph=False, encode_inline=True,
                      train_encoders=True, grad_clip=1e9, grad_accum_steps=2)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(16, seed=1), text_encoder=tenc, visual_encoder=venc)
    tr.fusion.load_state_dict(fus_sd); tr.clf.load_state_dict(clf_sd)
    tr.fusion.dropout = tr.clf.dropout = tr.clf.node_dropout = 0.0
    tr.head.step_bufs.clear()
    tr.fusion.train(); tr.clf.train()
    gb = {k: v.to(DEV) for k, v in batch.items()}
    gb.update({"input_ids": ids.to(DEV), "attention_mask": mask.to(torch.int32).to(DEV), "frames": frames.to(DEV)})
    tr.text_bp.refresh_operands(); tr.vis_bp.refresh_operands()      # (the first forward would build the operand copies lazily: not counted)
    refreshed = []
    for name, bp in (("text", tr.text_bp), ("vis", tr.vis_bp)):
        orig = bp.refresh_operands
        bp.refresh_operands = (lambda _o=orig, _n=name: (refreshed.append(_n), _o())[1])
    before = tr.arena.data.clone()
    losses = []
    for j in range(2):
        out = tr.train_step(_rows(gb, 2 * j, 2 * j + 2))
        losses.append(float(out["loss"].cpu()))
        if j == 0:
            assert refreshed == [] and torch.equal(tr.arena.data, before) and not tr._enc_dirty
            assert tr.optim.state.read().micro == 1
    st = tr.optim.state.read()
    assert sorted(refreshed) == ["text", "vis"] and tr._enc_dirty
    assert int(st.step) == 1 and st.micro == 0 and st.grad_scale == 0.5
    # oracle: autograd through encoders + head over the four rows
    wtl = {k: v.clone().requires_grad_(True) for k, v in wt.items()}
    wvl = {k: v.clone().requires_grad_(True) for k, v in wv.items()}
    fl = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in fus_sd.items()}
    cl = {k: v.clone().requires_grad_(v.is_floating_point() and not k.endswith("tau")) for k, v in clf_sd.items()}
    rb = dict(batch)
    rb["text_features"], rb["visual_features"] = E.text_features(wtl, ids, mask), E.visual_features(wvl, frames)
    ro = O.forward_batch(fl, cl, rb)
    loss = F.cross_entropy(ro["logits"], batch["label"])
    loss.backward()
    assert abs(sum(losses) / 2 - float(loss.detach())) <= 1e-3
    grads = {"text." + k: v.grad for k, v in wtl.items() if v.grad is not None}
    grads.update({"vis." + k: v.grad for k, v in wvl.items() if v.grad is not None})
    enc_norm = sum(float(g.double().pow(2).sum()) for g in grads.values()) ** 0.5
    head_norm = sum(float(v.grad.double().pow(2).sum()) for d in (fl, cl) for v in d.values() if v.requires_grad and v.grad is not None) ** 0.5
    total = (enc_norm ** 2 + head_norm ** 2) ** 0.5
    rel = abs(float(st.grad_norm) - total) / total
    print(f"mean micro-loss {sum(losses) / 2:.6f} (oracle {float(loss.detach()):.6f}); grad norm {float(st.grad_norm):.5f} (oracle {total:.5f})")
    print(f"global norm relative error {rel:.3e} (bound {ACCUM_NORM_REL:.1e})")
    _compare(tr.arena, float(st.grad_scale), grads, ENC_GRAD_REL, "2 x 2 rows accumulated, encoder gradients (2 + 2 layers behind the fp32 head)")
    assert rel <= ACCUM_NORM_REL
    moved = (tr.arena.data - before).abs().max().item()
    assert 0.0 < moved <= 1.05 * cfg.lr
