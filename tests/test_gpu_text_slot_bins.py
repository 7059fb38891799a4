"""GPU: the slot bins of the packed text pass (ufnd_text_pack_bins) and the fused Q/K/V + attention over them
(ufnd_qkv_attention_bf16_bins): the bin list is a partition of the live samples' 32-row slots, equal to the host-side
encoders.text_slot_bins, and the slot form's ctx equals the one-sample-per-workgroup packed form's bit for bit."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LQ = 128


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


def _n_rows(mask):
    m = mask.cpu().bool()
    return torch.where(m, torch.arange(m.shape[1])[None, :] + 1, 0).max(1).values.tolist()


def _bufs(B):
    i32 = dict(dtype=torch.int32, device=DEV)
    return {"cu": torch.full((B + 1,), -1, **i32), "row_src": torch.full((B * LQ,), -1, **i32),
            "bins": torch.full((B, 8), -7, **i32), "nbins": torch.full((1,), -7, **i32)}


def _pack(mask_d, b):
    L = _lib()
    B = mask_d.shape[0]
    L.check(L.lib().ufnd_text_pack_bins(mask_d.data_ptr(), B, LQ, b["cu"].data_ptr(), b["row_src"].data_ptr(), b["bins"].data_ptr(),
                                        b["nbins"].data_ptr(), L.stream_ptr(mask_d.device)), "ufnd_text_pack_bins")


def _descriptors(n_rows):
    """text_slot_bins in the device's format: slot (b, s) -> {cu[b] + 32 s, (b << 10) | (s << 8) | n_b}, empty -> {0, -1}"""
    from ultrafnd_git_amd.encoders import text_slot_bins
    cu = [0]
    for n in n_rows:
        cu.append(cu[-1] + n)
    out = []
    for bn in text_slot_bins(n_rows):
        row = []
        for x in bn:
            row += [0, -1] if x is None else [cu[x[0]] + 32 * x[1], (x[0] << 10) | (x[1] << 8) | n_rows[x[0]]]
        out.append(row)
    return torch.tensor(out, dtype=torch.int32).view(-1, 8)


def _check_bins(mask, b):
    """the device's bins against the host reference, and the partition rules on their own"""
    from ultrafnd_git_amd.encoders import text_slot_bin_count
    n_rows = _n_rows(mask)
    nb = int(b["nbins"].item())
    assert nb == text_slot_bin_count(n_rows)
    got = b["bins"][:nb].cpu()
    assert torch.equal(got, _descriptors(n_rows))
    seen, full_done = {}, False
    for i in range(nb):
        meta = got[i, 1::2].tolist()
        used = [m >= 0 for m in meta]
        assert used[0] and used == sorted(used, reverse=True), (i, meta)      # filled from slot 0 on
        full_done = full_done or not all(used)
        assert all(used) or full_done
        assert not (full_done and all(used)), "a full bin after a partial one"
        for j, m in enumerate(meta):
            if m >= 0:
                seen.setdefault(m >> 10, []).append((i, j, (m >> 8) & 3, m & 255))
    for s, n in enumerate(n_rows):
        c = (n + 31) // 32
        if c == 0:
            assert s not in seen
            continue
        sl = seen.pop(s)
        assert len({i for i, *_ in sl}) == 1 and [j for _, j, *_ in sl] == list(range(sl[0][1], sl[0][1] + c)), (s, sl)
        assert [x[2] for x in sl] == list(range(c)) and all(x[3] == n for x in sl)
    assert not seen
    return nb


def _mask(lens, holes=()):
    B = len(lens)
    mask = (torch.arange(LQ)[None, :] < torch.tensor(lens)[:, None]).int()
    for b, lo, hi in holes:
        mask[b, lo:hi] = 0
    return mask


def _mixes():
    g = torch.Generator().manual_seed(3)
    r = lambda B, lo, hi: torch.randint(lo, hi + 1, (B,), generator=g).tolist()
    border = [31, 32, 33, 63, 64, 65, 95, 96, 97, 128]
    return {
        "bench": (r(128, 16, 128), ()),
        "one_slot": (r(37, 1, 32), ()),
        "four_slot": (r(9, 97, 128), ()),
        "borders": (border, ()),
        "borders_shuffled_odd": ([border[i % 10] for i in torch.randperm(23, generator=g).tolist()], ()),
        "slot_border_holes": (border + [128, 70], ((0, 0, 31), (1, 31, 32), (3, 32, 63), (5, 64, 96), (9, 0, 64), (10, 30, 34),
                                                   (11, 0, 69), (9, 96, 127))),
        "B1_short": ([1], ()),
        "B1_mid": ([50], ()),
        "B1_full": ([128], ()),
        "single_one_slot_bin": ([10, 128, 128, 128, 128], ()),
        "three_without_partners": ([70, 80, 90, 5, 40], ()),
        "odd_two_and_one": ([40, 50, 60, 3], ()),
        "masked_and_odd": ([0, 17, 0, 64, 33, 0, 100, 1, 96, 0, 65], ()),
        "all_masked": ([0, 0, 0], ()),
    }


MIXES = _mixes()


@pytest.mark.parametrize("name", list(MIXES))
def test_bins_are_a_partition_equal_to_the_host_reference(name):
    lens, holes = MIXES[name]
    mask = _mask(lens, holes)
    b = _bufs(len(lens))
    _pack(mask.to(DEV), b)
    torch.cuda.synchronize()
    nb = _check_bins(mask, b)
    assert nb <= len(lens)
    if name == "all_masked":
        assert nb == 0


def test_bins_over_the_multi_sample_scan():
    """B = 5000 (more samples than the pack kernel's threads) and B = 16384 (its limit)"""
    g = torch.Generator().manual_seed(9)
    for B in (5000, 16384):
        lens = torch.randint(0, LQ + 1, (B,), generator=g)
        lens[torch.randperm(B, generator=g)[:B // 5]] = torch.randint(1, 33, (B // 5,), generator=g)
        mask = _mask(lens.tolist())
        b = _bufs(B)
        _pack(mask.to(DEV), b)
        torch.cuda.synchronize()
        _check_bins(mask, b)


def _operands(B, heads, seed, ln):
    g = torch.Generator().manual_seed(seed)
    H = heads * 64
    X = torch.randn(B * LQ, H, generator=g).bfloat16()
    W = (torch.randn(3 * H, H, generator=g) / H ** 0.5).bfloat16()
    bias = (torch.randn(3 * H, generator=g) * 0.1).float()
    ops = {"X": X.to(DEV), "W": W.to(DEV), "bias": bias.to(DEV)}
    if ln:      # partial {sum, sumsq} per 32 columns of the fp32 rows X was rounded from, and the weight's column sums
        xf = X.float().view(B * LQ, H // 32, 32)
        ops["st"] = torch.stack([xf.sum(2), (xf * xf).sum(2)], 2).contiguous().to(DEV)
        ops["colsum"] = W.float().sum(1).contiguous().to(DEV)
        ops["guard"] = torch.zeros(1024, dtype=torch.float32, device=DEV)
    return ops


def _qkv_attention(ops, mask_d, b, ctx, heads, bins):
    L = _lib()
    B = mask_d.shape[0]
    ln = None
    if "st" in ops:
        ln = L.GemmLn()
        ln.a_stats, ln.colsum, ln.a_parts, ln.a_eps, ln.r_eps, ln.width = ops["st"].data_ptr(), ops["colsum"].data_ptr(), ops["st"].shape[1], 1e-12, 1e-12, heads * 64
        ln.guard = ops["guard"].data_ptr()
    lnp = ctypes.byref(ln) if ln is not None else None
    s = L.stream_ptr(mask_d.device)
    X, W = ops["X"], ops["W"]
    if bins:
        L.check(L.lib().ufnd_qkv_attention_bf16_bins(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), mask_d.data_ptr(), b["cu"].data_ptr(),
                                                     b["bins"].data_ptr(), b["nbins"].data_ptr(), ctx.data_ptr(), B, LQ, heads, X.stride(0),
                                                     W.stride(0), lnp, s), "ufnd_qkv_attention_bf16_bins")
    else:
        L.check(L.lib().ufnd_qkv_attention_bf16_packed(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), mask_d.data_ptr(), b["cu"].data_ptr(),
                                                       ctx.data_ptr(), B, LQ, heads, X.stride(0), W.stride(0), lnp, s),
                "ufnd_qkv_attention_bf16_packed")


def _poisoned_ctx(B, heads):
    return torch.full((B * LQ, heads * 64), 0x7FC1, dtype=torch.int16, device=DEV).view(torch.bfloat16)


@pytest.mark.parametrize("heads,ln", [(2, False), (2, True), (12, False), (12, True)])
@pytest.mark.parametrize("name", list(MIXES))
def test_slot_form_ctx_equals_the_packed_form(name, heads, ln):
    lens, holes = MIXES[name]
    B = len(lens)
    mask = _mask(lens, holes)
    mask_d = mask.to(DEV)
    ops = _operands(B, heads, 60 + B, ln)
    b = _bufs(B)
    _pack(mask_d, b)
    want, got = _poisoned_ctx(B, heads), _poisoned_ctx(B, heads)
    _qkv_attention(ops, mask_d, b, want, heads, bins=False)
    if ln:
        g_want = ops["guard"].clone()
        ops["guard"].zero_()
    _qkv_attention(ops, mask_d, b, got, heads, bins=True)
    torch.cuda.synchronize()
    T = int(b["cu"][B].item())
    assert T == sum(_n_rows(mask))
    assert torch.equal(got.view(torch.int16)[:T], want.view(torch.int16)[:T]), name
    assert (got.view(torch.int16)[T:] == 0x7FC1).all(), "a row past the live rows was stored"
    if T:
        assert torch.isfinite(got[:T].float()).all()
    if ln:      # the fold guard covers the same (live) rows in both forms (its slots are per workgroup: compare the maxima)
        assert torch.equal(ops["guard"].max(), g_want.max())


def test_slot_form_in_a_captured_graph_over_rewritten_masks():
    """pack + slot-form launch captured once; the mask rewritten in place before each replay (bench mix, all 1-slot, all masked,
    all 4-slot): bins and ctx follow, equal to eager packed launches."""
    heads, B = 12, 40
    ops = _operands(B, heads, 77, True)
    mask_d = torch.zeros(B, LQ, dtype=torch.int32, device=DEV)
    mask_d.copy_(_mask([64] * B))
    b = _bufs(B)
    ctx = _poisoned_ctx(B, heads)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _pack(mask_d, b)
        _qkv_attention(ops, mask_d, b, ctx, heads, bins=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _pack(mask_d, b)
        _qkv_attention(ops, mask_d, b, ctx, heads, bins=True)
    g = torch.Generator().manual_seed(78)
    cases = [torch.randint(16, 129, (B,), generator=g).tolist(), torch.randint(1, 33, (B,), generator=g).tolist(), [0] * B,
             torch.randint(97, 129, (B,), generator=g).tolist(), MIXES["masked_and_odd"][0] * 3 + [10] * 7]
    for lens in cases:
        mask = _mask(lens, ((1, 31, 33), (2, 60, 70)))
        mask_d.copy_(mask)
        b["bins"].fill_(-7)
        ctx.view(torch.int16).fill_(0x7FC1)
        graph.replay()
        torch.cuda.synchronize()
        _check_bins(mask, b)
        ref_b = _bufs(B)
        _pack(mask_d, ref_b)
        want = _poisoned_ctx(B, heads)
        _qkv_attention(ops, mask_d, ref_b, want, heads, bins=False)
        torch.cuda.synchronize()
        T = int(ref_b["cu"][B].item())
        assert torch.equal(ctx.view(torch.int16)[:T], want.view(torch.int16)[:T]), lens
        assert (ctx.view(torch.int16)[T:] == 0x7FC1).all()
    del graph


@pytest.mark.parametrize("name", ["bench", "borders_shuffled_odd", "slot_border_holes", "single_one_slot_bin", "masked_and_odd"])
def test_text_encoder_over_slot_bins_equals_the_padded_pass(name):
    """BertTextEncoder's packed pass (now over slot bins) against unpad=False, features bit for bit."""
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import BertTextEncoder, text_slot_bin_count
    lens, holes = MIXES[name]
    enc = BertTextEncoder(layers=2, vocab_size=1000)
    enc.load_state_dict(E.seeded_weights(E.bert_shapes(layers=2, vocab=1000), 81))
    enc = enc.to(DEV)
    mask = _mask(lens, holes)
    ids = torch.randint(0, 1000, mask.shape, generator=torch.Generator().manual_seed(82))
    want = enc(ids, mask, unpad=False).clone()
    got = enc(ids, mask).clone()
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert int(enc._workbufs(len(lens), LQ)["nbins"].item()) == text_slot_bin_count(_n_rows(mask))
