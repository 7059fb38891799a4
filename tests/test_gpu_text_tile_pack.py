"""GPU: the sample tiles of the packed text pass (ufnd_text_pack_tiles) and the fused Q/K/V + attention over them
(ufnd_qkv_attention_bf16_tiles): the tile table equals the host-side encoders.text_tiles, and every live ctx row equals the padded
two-launch form's (ufnd_gemm_bf16[_ln] + ufnd_attention_bf16) and the slot-bin form's bit for bit."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LQ = 128
FILL = -7
POISON = 0x7FC1


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


def _n_rows(mask):
    m = mask.cpu().bool()
    return torch.where(m, torch.arange(m.shape[1])[None, :] + 1, 0).max(1).values.tolist()


def _mask(lens, holes=()):
    mask = (torch.arange(LQ)[None, :] < torch.tensor(lens)[:, None]).int()
    for b, lo, hi in holes:
        mask[b, lo:hi] = 0
    return mask


def _bufs(B):
    from ultrafnd_git_amd.encoders import TEXT_TILE_INTS
    i32 = dict(dtype=torch.int32, device=DEV)
    return {"cu": torch.full((B + 1,), -1, **i32), "row_src": torch.full((B * LQ,), -1, **i32),
            "tiles": torch.full(((B + 1) // 2, TEXT_TILE_INTS), FILL, **i32), "ntiles": torch.full((1,), FILL, **i32),
            "bins": torch.full((B, 8), FILL, **i32), "nbins": torch.full((1,), FILL, **i32)}


def _pack(mask_d, b, bins=True):
    L = _lib()
    B = mask_d.shape[0]
    L.check(L.lib().ufnd_text_pack_tiles(mask_d.data_ptr(), B, LQ, b["cu"].data_ptr(), b["row_src"].data_ptr(), b["tiles"].data_ptr(),
                                         b["ntiles"].data_ptr(), b["bins"].data_ptr() if bins else None, b["nbins"].data_ptr() if bins else None,
                                         L.stream_ptr(mask_d.device)), "ufnd_text_pack_tiles")


def _expected_table(mask):
    """encoders.text_tiles in the device's format (include/ultrafnd_hip.h); words the kernel leaves alone keep FILL"""
    from ultrafnd_git_amd import encoders as E
    n_rows = _n_rows(mask)
    cu = [0]
    for n in n_rows:
        cu.append(cu[-1] + n)
    tiles = E.text_tiles(n_rows)
    neg = torch.tensor([-3.0e38], dtype=torch.float32).view(torch.int32).item()
    out = torch.full((len(tiles), E.TEXT_TILE_INTS), FILL, dtype=torch.int32)
    for t, tl in enumerate(tiles):
        rows = sum(n_rows[b] for b, _ in tl)
        units = [j | (q << 8) for j, (b, _) in enumerate(tl) for q in range((n_rows[b] + 31) // 32)]
        out[t, :4] = torch.tensor([len(tl), rows, len(units), 0])
        out[t, E.TEXT_TILE_UNIT0:E.TEXT_TILE_UNIT0 + len(units)] = torch.tensor(units)
        out[t, E.TEXT_TILE_ROWMAP:E.TEXT_TILE_ROWMAP + 256] = cu[tl[0][0]]
        out[t, E.TEXT_TILE_KBIAS:E.TEXT_TILE_KBIAS + 256] = neg
        for j, (b, r0) in enumerate(tl):
            n = n_rows[b]
            out[t, 4 + 2 * j], out[t, 5 + 2 * j] = cu[b], (b << 16) | (r0 << 8) | n
            out[t, E.TEXT_TILE_ROWMAP + r0:E.TEXT_TILE_ROWMAP + r0 + n] = torch.arange(cu[b], cu[b] + n, dtype=torch.int32)
            out[t, E.TEXT_TILE_KBIAS + r0:E.TEXT_TILE_KBIAS + r0 + n] = torch.where(mask[b, :n] != 0, 0, neg).int()
    return out, cu


# (lengths, holes (b, lo, hi) masked inside a sample).  An all-masked sample has length 0 and takes no rows.
SETS = {
    "all_128": ([128] * 6, ()),
    "mixed": ([1, 15, 16, 17, 63, 64, 65, 127, 128, 0, 128, 64, 33, 0, 100, 2], ()),
    "mixed_holes": ([1, 15, 16, 17, 63, 64, 65, 127, 128, 0, 128, 64, 33, 0, 100, 2],
                    ((3, 0, 16), (4, 10, 11), (6, 0, 64), (7, 64, 126), (8, 0, 127), (10, 60, 70), (12, 1, 32), (14, 0, 99))),
    "sixteen_and_a_seventeenth": ([16, 3, 16, 1, 7, 16, 16, 9, 2, 16, 5, 16, 11, 16, 4, 13, 6], ((0, 3, 9), (7, 0, 8))),
    "short_beside_long": ([16, 3, 128, 1, 7, 16, 90, 9, 2, 16, 5, 16, 11, 16, 4, 13, 6, 1, 1, 1, 14], ()),
    "exactly_256": ([100, 128, 100, 56, 128], ((3, 20, 40),)),
    "B1": ([77], ()),
    "B1_full": ([128], ()),
    "all_masked": ([0, 0, 0], ()),
}


@pytest.mark.parametrize("name", list(SETS))
def test_tile_table_equals_the_host_mirror(name):
    from ultrafnd_git_amd.encoders import text_tile_count
    lens, holes = SETS[name]
    B = len(lens)
    mask = _mask(lens, holes)
    b = _bufs(B)
    _pack(mask.to(DEV), b)
    torch.cuda.synchronize()
    want, cu = _expected_table(mask)
    nt = int(b["ntiles"].item())
    assert nt == want.shape[0] == text_tile_count(_n_rows(mask))
    assert b["cu"].cpu().tolist() == cu
    assert torch.equal(b["tiles"][:nt].cpu(), want)
    assert (b["tiles"][nt:] == FILL).all(), "a tile past the count was written"
    if name == "all_128":
        assert nt == 3 and (b["tiles"][:nt, 0] == 2).all()
    if name == "sixteen_and_a_seventeenth":
        assert b["tiles"][:nt, 0].tolist() == [16, 1]
    if name == "exactly_256":
        assert b["tiles"][:nt, 1].tolist() == [256, 256]
    if name == "all_masked":
        assert nt == 0
    # the slot bins of the same launch are ufnd_text_pack_bins' own
    L = _lib()
    ref = _bufs(B)
    mask_d = mask.to(DEV)
    L.check(L.lib().ufnd_text_pack_bins(mask_d.data_ptr(), B, LQ, ref["cu"].data_ptr(), ref["row_src"].data_ptr(), ref["bins"].data_ptr(),
                                        ref["nbins"].data_ptr(), L.stream_ptr(mask_d.device)), "ufnd_text_pack_bins")
    torch.cuda.synchronize()
    for k in ("cu", "row_src", "bins", "nbins"):
        assert torch.equal(b[k], ref[k]), k


@pytest.mark.parametrize("what", ["129_mixed", "300_mixed", "512_full", "512_tiny", "512_mixed_holes"])
def test_tile_table_of_large_batches(what):
    """more than 128 samples: tiles past the first 64 (the pack kernel's general placement loop), up to the 512-sample limit"""
    g = torch.Generator().manual_seed(21)
    B = int(what.split("_")[0])
    lens = {"full": [128] * B, "tiny": torch.randint(1, 9, (B,), generator=g).tolist()}.get(what.split("_")[1]) or \
        torch.randint(0, 129, (B,), generator=g).tolist()
    mask = _mask(lens, ((1, 0, 5), (7, 3, 60)) if what.endswith("holes") else ())
    b = _bufs(B)
    _pack(mask.to(DEV), b, bins=False)
    torch.cuda.synchronize()
    want, cu = _expected_table(mask)
    nt = int(b["ntiles"].item())
    assert nt == want.shape[0] and b["cu"].cpu().tolist() == cu
    assert torch.equal(b["tiles"][:nt].cpu(), want)
    assert (b["tiles"][nt:] == FILL).all() and (b["bins"] == FILL).all()
    if what == "512_full":
        assert nt == 256


def test_pack_refuses_what_it_is_not_built_for():
    L = _lib()
    b = _bufs(4)
    m = torch.ones(4, LQ, dtype=torch.int32, device=DEV)
    args = (b["cu"].data_ptr(), b["row_src"].data_ptr(), b["tiles"].data_ptr(), b["ntiles"].data_ptr(), None, None, L.stream_ptr(m.device))
    assert L.lib().ufnd_text_pack_tiles(m.data_ptr(), 513, LQ, *args) == 1
    assert L.lib().ufnd_text_pack_tiles(m.data_ptr(), 4, 129, *args) == 1
    assert L.lib().ufnd_text_pack_tiles(m.data_ptr(), 4, LQ, *args[:4], b["bins"].data_ptr(), None, args[-1]) == 1


# ---------------------------------------------------------------------------------------------------------------------------- ctx
def _operands(B, heads, seed, ln):
    """the PADDED batch's operands: X (B * 128, H) and, with ln, the statistics of the fp32 rows it was rounded from"""
    g = torch.Generator().manual_seed(seed)
    H = heads * 64
    X = torch.randn(B * LQ, H, generator=g).bfloat16()
    W = (torch.randn(3 * H, H, generator=g) / H ** 0.5).bfloat16()
    bias = (torch.randn(3 * H, generator=g) * 0.1).float()
    ops = {"X": X.to(DEV), "W": W.to(DEV), "bias": bias.to(DEV), "heads": heads}
    if ln:
        xf = X.float().view(B * LQ, H // 32, 32)
        ops["st"] = torch.stack([xf.sum(2), (xf * xf).sum(2)], 2).contiguous().to(DEV)
        ops["colsum"] = W.float().sum(1).contiguous().to(DEV)
    return ops


def _ln(ops, st):
    L = _lib()
    if st is None:
        return None, None
    ln = L.GemmLn()
    ln.a_stats, ln.colsum, ln.a_parts, ln.a_eps, ln.r_eps, ln.width = st.data_ptr(), ops["colsum"].data_ptr(), st.shape[1], 1e-12, 1e-12, ops["heads"] * 64
    return ln, ctypes.byref(ln)


def _padded_two_launch(ops, mask_d):
    """ufnd_gemm_bf16[_ln] + ufnd_attention_bf16 on the padded batch: ctx (B * 128, H)"""
    L = _lib()
    B, heads = mask_d.shape[0], ops["heads"]
    H, M = heads * 64, mask_d.shape[0] * LQ
    X, W, s = ops["X"], ops["W"], L.stream_ptr(mask_d.device)
    qkv = torch.empty(M, 3 * H, dtype=torch.bfloat16, device=DEV)
    ctx = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    ln, lnp = _ln(ops, ops.get("st"))
    if ln is not None:
        L.check(L.lib().ufnd_gemm_bf16_ln(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), None, qkv.data_ptr(), None, M, 3 * H, H, H, H, 0, 3 * H, 0, 0,
                                          lnp, s), "ufnd_gemm_bf16_ln")
    else:
        L.check(L.lib().ufnd_gemm_bf16(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), None, qkv.data_ptr(), None, M, 3 * H, H, H, H, 0, 3 * H, 0, 0, s),
                "ufnd_gemm_bf16")
    L.check(L.lib().ufnd_attention_bf16(qkv.data_ptr(), mask_d.data_ptr(), ctx.data_ptr(), B, LQ, heads, s), "ufnd_attention_bf16")
    return ctx


def _gather(ops, b, into=None):
    """the packed operands: row r is row row_src[r] of the padded batch (rows past the live ones: zeros)"""
    T = int(b["cu"][-1].item())
    src = b["row_src"][:T].long()
    out = into or {"X": torch.zeros_like(ops["X"]), "st": torch.zeros_like(ops["st"]) if "st" in ops else None}
    for k in ("X", "st"):
        if out[k] is not None:
            out[k].zero_()
            out[k][:T] = ops[k][src]
    return out, T


def _poisoned_ctx(B, heads):
    return torch.full((B * LQ, heads * 64), POISON, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _tiles_launch(ops, pk, b, ctx):
    L = _lib()
    _, lnp = _ln(ops, pk["st"])
    X, W = pk["X"], ops["W"]
    L.check(L.lib().ufnd_qkv_attention_bf16_tiles(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), b["tiles"].data_ptr(), b["ntiles"].data_ptr(),
                                                  ctx.data_ptr(), b["tiles"].shape[0], ops["heads"], X.stride(0), W.stride(0), lnp,
                                                  L.stream_ptr(X.device)), "ufnd_qkv_attention_bf16_tiles")


def _bins_launch(ops, pk, mask_d, b, ctx):
    L = _lib()
    _, lnp = _ln(ops, pk["st"])
    X, W = pk["X"], ops["W"]
    L.check(L.lib().ufnd_qkv_attention_bf16_bins(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), mask_d.data_ptr(), b["cu"].data_ptr(),
                                                 b["bins"].data_ptr(), b["nbins"].data_ptr(), ctx.data_ptr(), mask_d.shape[0], LQ, ops["heads"],
                                                 X.stride(0), W.stride(0), lnp, L.stream_ptr(X.device)), "ufnd_qkv_attention_bf16_bins")


def _live_rows_of_padded(ctx_pad, b, T):
    return ctx_pad[b["row_src"][:T].long()]


@pytest.mark.parametrize("heads,ln", [(2, False), (2, True), (4, False), (4, True)])
@pytest.mark.parametrize("name", list(SETS))
def test_tile_form_ctx_equals_the_padded_two_launch_form(name, heads, ln):
    lens, holes = SETS[name]
    B = len(lens)
    mask = _mask(lens, holes)
    mask_d = mask.to(DEV)
    ops = _operands(B, heads, 160 + B, ln)
    b = _bufs(B)
    _pack(mask_d, b)
    pk, T = _gather(ops, b)
    assert T == sum(_n_rows(mask))
    want = _live_rows_of_padded(_padded_two_launch(ops, mask_d), b, T)
    got, slot = _poisoned_ctx(B, heads), _poisoned_ctx(B, heads)
    _tiles_launch(ops, pk, b, got)
    _bins_launch(ops, pk, mask_d, b, slot)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16)[:T], want.view(torch.int16)), name
    assert torch.equal(got.view(torch.int16), slot.view(torch.int16)), name
    assert (got.view(torch.int16)[T:] == POISON).all(), "a row past the live rows was stored"
    if T:
        assert torch.isfinite(got[:T].float()).all()


def test_tile_form_leaves_the_fold_guard_of_the_live_rows():
    """the largest |mean| / std the folded launch reports is the live rows' -- a clamped or hole row never adds to it"""
    lens, holes = SETS["mixed_holes"]
    B, heads = len(lens), 2
    mask_d = _mask(lens, holes).to(DEV)
    ops = _operands(B, heads, 31, True)
    b = _bufs(B)
    _pack(mask_d, b)
    pk, T = _gather(ops, b)
    L = _lib()
    maxima = []
    for launch in ("tiles", "bins"):
        guard = torch.zeros(1024, dtype=torch.float32, device=DEV)
        ln, lnp = _ln(ops, pk["st"])
        ln.guard = guard.data_ptr()
        ctx = _poisoned_ctx(B, heads)
        X, W = pk["X"], ops["W"]
        if launch == "tiles":
            L.check(L.lib().ufnd_qkv_attention_bf16_tiles(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), b["tiles"].data_ptr(),
                                                          b["ntiles"].data_ptr(), ctx.data_ptr(), b["tiles"].shape[0], heads, X.stride(0), W.stride(0),
                                                          lnp, L.stream_ptr(X.device)), "ufnd_qkv_attention_bf16_tiles")
        else:
            L.check(L.lib().ufnd_qkv_attention_bf16_bins(X.data_ptr(), W.data_ptr(), ops["bias"].data_ptr(), mask_d.data_ptr(), b["cu"].data_ptr(),
                                                         b["bins"].data_ptr(), b["nbins"].data_ptr(), ctx.data_ptr(), B, LQ, heads, X.stride(0),
                                                         W.stride(0), lnp, L.stream_ptr(X.device)), "ufnd_qkv_attention_bf16_bins")
        torch.cuda.synchronize()
        maxima.append(guard.max())
    assert maxima[0] > 0 and torch.equal(maxima[0], maxima[1])


def test_tile_form_in_a_captured_graph_over_rewritten_inputs():
    """pack + tile-form launch captured once; mask, rows and statistics rewritten in place before each replay: the table and ctx follow"""
    heads, B = 4, 24
    ops = _operands(B, heads, 177, True)
    mask_d = torch.zeros(B, LQ, dtype=torch.int32, device=DEV)
    mask_d.copy_(_mask([64] * B))
    b = _bufs(B)
    pk = {"X": torch.zeros_like(ops["X"]), "st": torch.zeros_like(ops["st"])}      # the captured launch's packed operands
    ctx = _poisoned_ctx(B, heads)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _pack(mask_d, b)
        _tiles_launch(ops, pk, b, ctx)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _pack(mask_d, b)
        _tiles_launch(ops, pk, b, ctx)
    g = torch.Generator().manual_seed(178)
    cases = [torch.randint(16, 129, (B,), generator=g).tolist(), torch.randint(1, 17, (B,), generator=g).tolist(), [0] * B, [128] * B,
             SETS["mixed"][0] + [0, 5, 0, 128, 31, 0, 96, 40]]
    for lens in cases:
        mask = _mask(lens, ((1, 31, 33), (2, 60, 70)))
        mask_d.copy_(mask)
        ref_b = _bufs(B)
        _pack(mask_d, ref_b)
        _gather(ops, ref_b, into=pk)      # (the captured launch's own operand buffers, rewritten in place)
        b["tiles"].fill_(FILL)
        ctx.view(torch.int16).fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        want_table, _ = _expected_table(mask)
        nt = int(b["ntiles"].item())
        assert nt == want_table.shape[0] and torch.equal(b["tiles"][:nt].cpu(), want_table)
        T = int(ref_b["cu"][B].item())
        want = _live_rows_of_padded(_padded_two_launch(ops, mask_d), ref_b, T)
        torch.cuda.synchronize()
        assert torch.equal(ctx.view(torch.int16)[:T], want.view(torch.int16)), lens
        assert (ctx.view(torch.int16)[T:] == POISON).all()
    del graph


def test_text_encoder_over_sample_tiles_equals_slot_bins_and_the_padded_pass():
    """BertTextEncoder's packed pass over sample tiles (the default) against the pass over slot bins and against unpad=False"""
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import BertTextEncoder, text_slot_bin_count, text_tile_count
    lens, holes = [128, 17, 64, 0, 100, 65, 1, 33, 128, 90, 16, 127], ((2, 0, 10), (4, 50, 70))
    enc = BertTextEncoder(layers=2, vocab_size=1000)
    enc.load_state_dict(E.seeded_weights(E.bert_shapes(layers=2, vocab=1000), 81))
    enc = enc.to(DEV)
    assert enc.text_sample_tiles
    enc.text_tile_min_grid = 0      # (the default keeps a batch this small on the slot bins)
    mask = _mask(lens, holes)
    ids = torch.randint(0, 1000, mask.shape, generator=torch.Generator().manual_seed(82))
    padded = enc(ids, mask, unpad=False).clone()
    tiles = enc(ids, mask).clone()
    wb = enc._workbufs(len(lens), LQ)
    assert int(wb["ntiles"].item()) == text_tile_count(_n_rows(mask))
    assert int(wb["nbins"].item()) == text_slot_bin_count(_n_rows(mask))
    enc.text_sample_tiles = False
    wb["ntiles"].fill_(FILL)
    slots = enc(ids, mask).clone()
    assert int(wb["ntiles"].item()) == FILL, "the slot-bin pass ran the tile pack"
    assert torch.equal(tiles, padded), (tiles - padded).abs().max().item()
    assert torch.equal(tiles, slots)
