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
