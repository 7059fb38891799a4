"""GPU: the frozen text encoder's packed pass (BertTextEncoder.forward, unpad=True, the default) against the padded
computation (unpad=False), bit for bit.  The packed pass keeps each sample's positions 0 .. its last kept position as rows,
with the live row count on the device only (ufnd_text_pack); every kept row is computed exactly as in the padded batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _encoder(layers=2, fold=True, residual="bf16", fused=True, seed=71):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import BertTextEncoder
    enc = BertTextEncoder(layers=layers, vocab_size=1000, fold_ln=fold, residual_dtype=residual)
    enc.load_state_dict(E.seeded_weights(E.bert_shapes(layers=layers, vocab=1000), seed))
    enc.fuse_qkv_attention = fused
    return enc.to(DEV)


def _batch(B, Lq, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 1000, (B, Lq), generator=g)
    lens = torch.randint(lo, hi + 1, (B,), generator=g)
    mask = (torch.arange(Lq)[None, :] < lens[:, None]).int()
    return ids, mask


def _edge_rows(mask):
    """length-1 rows, an all-masked row, inner holes (one of them over a whole 64-key block) -- in place."""
    mask[0] = 0
    mask[1] = 0
    mask[1, 0] = 1
    mask[2, :] = 0
    mask[2, 5] = 1          # one kept token at position 5: rows 0 .. 5, five of them masked keys
    mask[3, 10:20] = 0
    mask[4, :] = 1
    mask[4, :70] = 0        # the first key block wholly masked
    return mask


def _check(enc, ids, mask):
    padded = enc(ids, mask, unpad=False).clone()
    packed = enc(ids, mask).clone()
    assert torch.equal(packed, padded), (packed - padded).abs().max().item()
    return packed


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("residual", ["bf16", "fp32"])
@pytest.mark.parametrize("fold", [True, False])
def test_packed_equals_padded_at_the_bench_group_shape(fold, residual, fused):
    """B = 128, L = 128, lengths uniform in [16, 128] (the bench's lookahead group), plus edge rows."""
    enc = _encoder(fold=fold, residual=residual, fused=fused)
    ids, mask = _batch(128, 128, 16, 128, 5)
    mask = _edge_rows(mask)
    out = _check(enc, ids, mask)
    assert torch.equal(out[0], torch.zeros_like(out[0]))
    # the live row count the pack kernel left on the device
    last = torch.where(mask.bool(), torch.arange(128)[None, :] + 1, 0).max(1).values
    cu = enc._workbufs(128, 128)["cu"].cpu()
    assert torch.equal(cu[1:] - cu[:-1], last.int()) and int(cu[-1]) == int(last.sum())
    assert int(cu[-1]) % 256 != 0


@pytest.mark.parametrize("fold", [True, False])
def test_packed_equals_padded_with_every_row_full(fold):
    enc = _encoder(fold=fold)
    ids, mask = _batch(16, 128, 128, 128, 6)
    _check(enc, ids, mask)


def test_packed_equals_padded_at_512_tokens():
    """L = 512 (the two-launch path: live-row Q/K/V GEMM + masked varlen attention)."""
    enc = _encoder(layers=2)
    ids, mask = _batch(3, 512, 1, 512, 7)
    mask[0, :] = 1
    mask[1, 100:300] = 0
    mask[1, 400] = 1
    _check(enc, ids, mask)


def test_packed_equals_padded_with_twelve_layers():
    enc = _encoder(layers=12, seed=3)
    ids, mask = _batch(32, 128, 16, 128, 8)
    _check(enc, ids, mask)


def test_captured_packed_pass_follows_rewritten_inputs():
    """One graph captured over the packed pass; ids and mask rewritten in place with a larger and a smaller token count: each
    replay equals a fresh padded eager run."""
    enc = _encoder(layers=3)
    B, Lq = 64, 128
    ids0, mask0 = _batch(B, Lq, 40, 80, 9)
    ids_d, mask_d = ids0.to(DEV), mask0.to(DEV, torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(ids_d, mask_d)          # warm-up: packs the weights, allocates the work buffers
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(ids_d, mask_d)
    for seed, lo, hi in ((10, 40, 80), (11, 100, 128), (12, 1, 20)):
        ids, mask = _batch(B, Lq, lo, hi, seed)
        mask[5, 3:9] = 0
        ids_d.copy_(ids)
        mask_d.copy_(mask)
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        want = enc(ids, mask, unpad=False).clone()
        assert torch.equal(got, want), (seed, (got - want).abs().max().item())


# ---------------------------------------------------------------------------------------- every length, capacity and live row count
def _edge_rows_any(mask):
    """_edge_rows for any length: all-masked first and middle samples, a length-1 one, a single kept token past holes, a hole, a full
    one, and (L > 70) the first 64-key block wholly masked -- in place."""
    B, Lq = mask.shape
    mask[0] = 0
    mask[1] = 0
    mask[1, 0] = 1
    mask[2] = 0
    mask[2, min(5, Lq - 1)] = 1
    mask[3, Lq // 4: Lq // 2] = 0
    mask[4] = 1
    if B > 7:
        mask[6] = 0
    if Lq > 70 and B > 5:
        mask[5] = 1
        mask[5, :70] = 0
    return mask


def _poison_workbufs(enc, B, Lq):
    """every work buffer of the (B, Lq) pass: NaN (fp32), a bf16 NaN pattern, -1 (int32)"""
    for t in enc._workbufs(B, Lq).values():
        if t.dtype == torch.int32:
            t.fill_(-1)
        elif t.dtype == torch.bfloat16:
            t.view(torch.int16).fill_(0x7FC1)
        else:
            t.fill_(float("nan"))


@pytest.mark.parametrize("Lq,B", [(1, 9), (40, 13), (77, 11), (200, 7), (256, 9)])
def test_packed_equals_padded_at_every_length(Lq, B):
    """L = 1 .. 256 (the reference's max_length): the two-launch path, the short-sequence attention kernels (L <= 64), a capacity
    B L that is not a multiple of 256, edge rows."""
    assert Lq % 256 == 0 or (B * Lq) % 256 != 0
    enc = _encoder(layers=2)
    ids, mask = _batch(B, Lq, 1, Lq, 20 + Lq)
    if Lq > 1:
        mask = _edge_rows_any(mask)
    else:
        mask[::3] = 0
    _check(enc, ids, mask)


def test_packed_equals_padded_at_the_configs3_geometry():
    """configs[3]: 12 layers, vocab 30522, B = 128, L = 512 (65,536 rows: the persistent GEMM runs Q/K/V, FFN1 and the LayerNorm-residual
    out-projection over live rows), variable lengths, on both residual streams."""
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import BertTextEncoder
    w = E.seeded_weights(E.bert_shapes(layers=12, vocab=30522), 4)
    ids, mask = E.synthetic_tokens(44, 128, 512, vocab=30522, min_len=1)
    mask[7, 100:300] = 0
    mask[9] = 0
    for residual in ("bf16", "fp32"):
        enc = BertTextEncoder(layers=12, vocab_size=30522, residual_dtype=residual)
        enc.load_state_dict(w)
        enc = enc.to(DEV)
        out = _check(enc, ids, mask)
        assert torch.isfinite(out).all()
        del enc
        torch.cuda.empty_cache()


def test_all_masked_batch_and_the_multi_sample_scan():
    """An all-masked batch (no live row at all) gives zero, finite features equal to the padded pass; B = 1500 at L = 16 runs the
    pack kernel's multi-sample scan (more samples than threads) through the whole pass."""
    enc = _encoder(layers=2)
    ids, mask = _batch(6, 128, 1, 128, 30)
    mask.zero_()
    out = _check(enc, ids, mask)
    assert torch.equal(out, torch.zeros_like(out))
    ids, mask = _batch(1500, 16, 1, 16, 31)
    mask[::7] = 0
    mask[1::11, 3:9] = 0
    _check(enc, ids, mask)


@pytest.mark.parametrize("Lq,fused,fold,residual", [(128, fu, fo, r) for fu in (True, False) for fo in (True, False) for r in ("bf16", "fp32")]
                         + [(256, False, True, "bf16"), (512, False, True, "fp32")])
def test_packed_pass_over_poisoned_work_buffers(Lq, fused, fold, residual):
    """The padded pass leaves plausible values in the shared work buffers; poisoned instead, a dead row read through a zero-weight path
    (a masked key, a clamped load) turns a live feature into NaN.  After poisoning, the packed pass still equals the padded features."""
    enc = _encoder(fold=fold, residual=residual, fused=fused)
    B = {128: 24, 256: 9, 512: 6}[Lq]
    ids, mask = _batch(B, Lq, 1, Lq, 40 + Lq)
    mask = _edge_rows_any(mask)
    mask[-1] = 0
    mask[-1, :Lq // 3] = 1      # the last sample ends inside a tile: its clamped loads reach the dead rows
    want = enc(ids, mask, unpad=False).clone()
    _poison_workbufs(enc, B, Lq)
    got = enc(ids, mask).clone()
    assert torch.equal(got, want), (Lq, fused, fold, residual, (got - want).abs().max().item())


def test_captured_packed_pass_over_poisoned_work_buffers():
    """The captured packed pass, every work buffer poisoned before each replay; the live row count goes 0 -> full -> small."""
    enc = _encoder(layers=3)
    B, Lq = 32, 128
    ids0, mask0 = _batch(B, Lq, 40, 80, 50)
    ids_d, mask_d = ids0.to(DEV), mask0.to(DEV, torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(ids_d, mask_d)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(ids_d, mask_d)
    for what, lo, hi in (("none", 0, 0), ("full", 128, 128), ("small", 1, 9)):
        ids, mask = _batch(B, Lq, max(lo, 1), max(hi, 1), 51)
        if what == "none":
            mask.zero_()
        ids_d.copy_(ids)
        mask_d.copy_(mask)
        _poison_workbufs(enc, B, Lq)
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        want = enc(ids, mask, unpad=False).clone()
        assert torch.equal(got, want), (what, (got - want).abs().max().item())
    del graph


def test_fold_guard_of_the_packed_pass():
    """The padded pass folds a superset of the packed pass's rows: its guard is never smaller, and equal when no sample has trailing
    padding."""
    enc = _encoder(layers=3, fold=True)
    for what, lo in (("padded", 5), ("full", 128)):
        ids, mask = _batch(32, 128, lo, 128, 60)
        if what == "full":
            mask[3, 10:40] = 0      # holes stay rows: still no trailing padding
        ratios = []
        for unpad in (False, True):
            enc._guard_buf(torch.device(DEV)).zero_()
            enc(ids, mask, unpad=unpad)
            ratios.append(enc.fold_ratio())
        padded, packed = ratios
        assert 0.0 < packed <= padded, (what, packed, padded)
        if what == "full":
            assert packed == padded, (packed, padded)


def _trainer_runs(tmp_path, padded):
    """train_group_pipelined over two groups (the second partial) and one plain epoch loop, with the text encoder's forward bound to
    the packed (default) or the padded pass: (logits, per-step losses, arena, epoch result, pipeline stats)."""
    import functools
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    B, G = 4, 3
    tenc = BertTextEncoder(layers=2, vocab_size=500)
    tenc.load_state_dict(E.seeded_weights(E.bert_shapes(layers=2, vocab=500), 11))
    venc = ClipVisualEncoder(layers=1)
    venc.load_state_dict(E.seeded_weights(E.vit_shapes(layers=1), 12))
    tenc, venc = tenc.to(DEV), venc.to(DEV)
    if padded:
        tenc.forward = functools.partial(BertTextEncoder.forward, tenc, unpad=False)
    g = torch.Generator().manual_seed(2)

    def macro(seed):
        ids, mask = E.synthetic_tokens(seed, G * B, 128, vocab=500, min_len=1)
        mask[1] = 0
        mask[G * B - 2] = 0
        mask[5, 3:20] = 0
        return {"input_ids": ids.to(DEV), "attention_mask": mask.to(torch.int32).to(DEV),
                "frames": torch.randn(G * B, 1, 3, 224, 224, generator=g).to(DEV), "audio_features": torch.randn(G * B, 128, generator=g).to(DEV),
                "temporal_features": torch.randn(G * B, 256, generator=g).to(DEV), "gnn_feat": torch.randn(G * B, 128, generator=g).to(DEV),
                "aux": torch.rand(G * B, 2, generator=g).to(DEV), "label": torch.randint(0, 2, (G * B,), generator=g).to(DEV)}
    groups = [macro(31), macro(32)]
    torch.manual_seed(7)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path / f"p{int(padded)}"), batch_size=B, device=DEV, encode_inline=True)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(48, seed=2, with_raw=True, seq_len=128, vocab=500), text_encoder=tenc, visual_encoder=venc)
    tr.fusion.train(); tr.clf.train()
    tr.prefetch_features(groups[0], group=True)
    out = tr.train_group_pipelined(groups[0], groups[1])
    losses = [float(x.cpu()) for x in out["losses"]]
    out = tr.train_group_pipelined(groups[1], None, steps=2)
    losses += [float(x.cpu()) for x in out["losses"]]
    torch.cuda.synchronize()
    logits, arena = out["logits"].clone(), tr.arena.data.clone()
    ep = tr._epoch_loop(tr.train_loader, "train")
    torch.cuda.synchronize()
    return logits, losses, arena, ep, tr.arena.data.clone(), dict(tr.pipe.stats)


def test_trainer_with_packed_text_equals_the_padded_pass(tmp_path):
    """The captured encoder passes inside the training step over packed text leave the same logits, per-step losses and parameter arena
    as the padded pass -- the lookahead groups (samples of one kept token and all-masked samples included) and a plain epoch loop."""
    a = _trainer_runs(tmp_path, padded=False)
    b = _trainer_runs(tmp_path, padded=True)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and len(a[1]) == 5, (a[1], b[1])
    assert torch.equal(a[2], b[2])
    assert repr(a[3]) == repr(b[3]) and torch.equal(a[4], b[4])
    for st in (a[5], b[5]):
        assert st["pinned_replays"] + st["staged_replays"] > 0 and st["fold_trips"] == 0, st
