"""The ViT's fused Q/K/V projection + attention launch (ufnd_qkv_attention_bf16_vit: 256 // T whole samples of T <= 64 rows and one
head per workgroup) against the two-launch form, ufnd_gemm_bf16[_ln] into qkv followed by ufnd_attention_bf16: ctx bit for bit, at
the op level (partial / exact / straddling row tiles, K shorter than the operand ring, folded LayerNorm, bias), with poisoned
surroundings, and through ClipVisualEncoder (eager and captured).  The argument checks run without a GPU."""
import ctypes as C
import functools

import pytest
import torch

DEV = "cuda"
gpu = pytest.mark.gpu
EPS = 1e-5


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


def _split_stats(x, parts):
    """(M, H) fp32 -> (M, parts, 2) partial {sum, sumsq} over `parts` equal column slices."""
    M, H = x.shape
    xs = x.view(M, parts, H // parts)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).contiguous()


@functools.lru_cache(maxsize=None)
def _operands(N, T, heads, with_ln, with_bias):
    """Seeded Gaussian operands (the scale of test_gpu_tier_b's fused-attention test) and the two-launch ctx, computed once per case
    and left unchanged."""
    L = _lib()
    H, M = heads * 64, N * T
    g = torch.Generator().manual_seed(1000 * N + 10 * T + heads)
    x = (torch.randn(M, H, generator=g) * 1.3 + 0.1).to(DEV)
    Wf = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(3 * H, generator=g)).to(DEV)
    ops = {"N": N, "T": T, "heads": heads, "H": H, "M": M, "st": None, "cs": None, "parts": 0}
    if with_ln:
        gm, bt = (1 + 0.2 * torch.randn(H, generator=g)).to(DEV), (0.1 * torch.randn(H, generator=g)).to(DEV)
        W = (Wf * gm[None, :]).bfloat16()
        ops["parts"] = 24 if H % 24 == 0 else 2
        ops["cs"], ops["st"] = W.float().sum(1).contiguous(), _split_stats(x, ops["parts"])
        b2 = (bias + Wf @ bt).contiguous()
    else:
        W, b2 = Wf.bfloat16(), bias
    ops["xb"], ops["W"], ops["bias"] = x.bfloat16(), W, (b2 if with_bias else None)
    qkv = torch.empty(M, 3 * H, dtype=torch.bfloat16, device=DEV)
    want = torch.empty(M, H, dtype=torch.bfloat16, device=DEV)
    s = L.stream_ptr(x.device)
    if with_ln:
        ln = _ln(ops, ops["st"])
        L.check(L.lib().ufnd_gemm_bf16_ln(ops["xb"].data_ptr(), W.data_ptr(), L.ptr(ops["bias"]), None, qkv.data_ptr(), None, M, 3 * H, H, H, H,
                                          0, 3 * H, 0, 0, C.byref(ln), s), "gemm_ln")
    else:
        L.check(L.lib().ufnd_gemm_bf16(ops["xb"].data_ptr(), W.data_ptr(), L.ptr(ops["bias"]), None, qkv.data_ptr(), None, M, 3 * H, H, H, H,
                                       0, 3 * H, 0, 0, s), "gemm")
    L.check(L.lib().ufnd_attention_bf16(qkv.data_ptr(), None, want.data_ptr(), N, T, heads, s), "attention")
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all()
    ops["want"] = want
    return ops


def _ln(ops, st):
    L = _lib()
    ln = L.GemmLn()
    ln.a_stats, ln.colsum, ln.a_parts, ln.a_eps, ln.r_eps, ln.width = st.data_ptr(), ops["cs"].data_ptr(), ops["parts"], EPS, EPS, ops["H"]
    return ln


def _fused(ops, x, st, ctx):
    L = _lib()
    ln = _ln(ops, st) if st is not None else None
    return L.lib().ufnd_qkv_attention_bf16_vit(x.data_ptr(), ops["W"].data_ptr(), L.ptr(ops["bias"]), ctx.data_ptr(), ops["N"], ops["T"],
                                               ops["heads"], x.stride(0), ops["W"].stride(0), C.byref(ln) if ln is not None else None,
                                               L.stream_ptr(x.device))


def _check_op(N, T, heads, with_ln, with_bias):
    L = _lib()
    ops = _operands(N, T, heads, with_ln, with_bias)
    ctx = torch.full((ops["M"], ops["H"]), float("nan"), dtype=torch.bfloat16, device=DEV)
    L.check(_fused(ops, ops["xb"], ops["st"], ctx), "ufnd_qkv_attention_bf16_vit")
    torch.cuda.synchronize()
    assert torch.isfinite(ctx.float()).all()
    assert torch.equal(ctx, ops["want"]), (ctx.float() - ops["want"].float()).abs().max().item()


@gpu
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("with_ln", [False, True])
@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("N", [1, 4, 5, 6, 11])
def test_ctx_is_bit_identical_to_gemm_plus_attention(N, heads, with_ln, with_bias):
    """T = 50, five samples per row tile: one sample, a partial tile, an exact tile, one sample into the second tile, two tiles and
    one sample; heads = 2 is K = 128, two K-steps for a three-slot ring."""
    _check_op(N, 50, heads, with_ln, with_bias)


@gpu
@pytest.mark.parametrize("with_ln", [False, True])
@pytest.mark.parametrize("N,T", [(9, 64), (13, 37), (11, 31), (20, 17), (300, 1)])
def test_other_sample_lengths(N, T, with_ln):
    """T = 64 (no key past T: the softmax's short path, four samples fill the tile exactly), T = 37 and 17 (6 and 15 samples per tile,
    256 is no multiple of them), T = 31 (one query block whose second 16-query tile lacks its last query), T = 1 (256 one-row samples
    per tile)."""
    _check_op(N, T, 12, with_ln, True)


@gpu
@pytest.mark.parametrize("with_ln", [False, True])
@pytest.mark.parametrize("N", [6, 11])
def test_nothing_past_the_last_row_is_read_or_written(N, with_ln):
    """X (and the row statistics) are views of larger buffers whose rows past N T hold NaN, ctx a view of a larger buffer holding a
    canary: the same ctx, no NaN, the canary intact."""
    L = _lib()
    ops = _operands(N, 50, 12, with_ln, True)
    M, H, pad = ops["M"], ops["H"], 300
    xbig = torch.full((M + pad, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    xbig[:M] = ops["xb"]
    st = None
    if with_ln:
        stbig = torch.full((M + pad, ops["parts"], 2), float("nan"), device=DEV)
        stbig[:M] = ops["st"]
        st = stbig[:M]
    cbig = torch.empty(pad + M + pad, H, dtype=torch.bfloat16, device=DEV)
    cbig.view(torch.int16).fill_(0x7FC1)
    ctx = cbig[pad:pad + M]
    guard = torch.zeros(L.FOLD_GUARD_SLOTS, device=DEV)
    ln = None
    if with_ln:
        ln = _ln(ops, st)
        ln.guard = guard.data_ptr()
    L.check(L.lib().ufnd_qkv_attention_bf16_vit(xbig.data_ptr(), ops["W"].data_ptr(), ops["bias"].data_ptr(), ctx.data_ptr(), N, 50, 12, H, H,
                                                C.byref(ln) if ln is not None else None, L.stream_ptr(xbig.device)), "ufnd_qkv_attention_bf16_vit")
    torch.cuda.synchronize()
    assert torch.isfinite(ctx.float()).all()
    assert torch.equal(ctx, ops["want"])
    bits = cbig.view(torch.int16)
    assert (bits[:pad] == 0x7FC1).all() and (bits[pad + M:] == 0x7FC1).all()
    assert torch.isfinite(guard).all()      # (the fold guard saw live rows only)


def _encoder(fold, residual, layers=2):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    enc = ClipVisualEncoder(layers=layers, fold_ln=fold, residual_dtype=residual)
    enc.load_state_dict(E.seeded_weights(E.vit_shapes(layers=layers), 62))
    return enc.to(DEV)


@gpu
@pytest.mark.parametrize("residual", ["bf16", "fp32"])
@pytest.mark.parametrize("fold", [True, False])
def test_visual_encoder_fused_equals_two_launch(fold, residual):
    from oracle import encoders_ref as E
    enc = _encoder(fold, residual)
    assert enc.fuse_qkv_attention
    for B, Fr in ((3, 1), (7, 1), (2, 2)):
        frames = E.synthetic_frames(40 + B, B, Fr)
        enc.fuse_qkv_attention = True
        a_f, a_h = enc(frames).clone(), enc.hidden_state(frames).clone()
        enc.fuse_qkv_attention = False
        b_f, b_h = enc(frames).clone(), enc.hidden_state(frames).clone()
        assert torch.isfinite(a_f).all() and torch.isfinite(a_h).all()
        assert torch.equal(a_f, b_f) and torch.equal(a_h, b_h), (B, Fr)


@gpu
def test_visual_encoder_fused_in_a_captured_graph():
    """The fused pass captured once and replayed twice with the frames rewritten in between: each replay equals the eager two-launch
    pass on the same frames."""
    from oracle import encoders_ref as E
    enc = _encoder(True, "bf16")
    B = 7
    frames = E.synthetic_frames(51, B, 1).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(frames)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(frames)
    ref = _encoder(True, "bf16")
    ref.fuse_qkv_attention = False
    for seed in (52, 53):
        fr = E.synthetic_frames(seed, B, 1).to(DEV)
        frames.copy_(fr)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = ref(fr)
        assert torch.isfinite(out).all() and torch.equal(out, want), seed
    del graph


def test_refusals():
    """Argument checks (no launch, so no GPU): null operands, T outside 1 .. 64 named with a pointer to the two-launch form, misaligned
    strides and pointers."""
    L = _lib()
    f = L.lib().ufnd_qkv_attention_bf16_vit
    buf = torch.zeros(1 << 16, dtype=torch.int16)
    p = buf.data_ptr()
    assert p % 16 == 0
    H = 128
    ok = dict(X=p, W=p, b=p, ctx=p, N=3, T=50, heads=2, ldx=H, ldw=H)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["X"], a["W"], a["b"], a["ctx"], a["N"], a["T"], a["heads"], a["ldx"], a["ldw"], None, None)

    for kw in (dict(X=None), dict(W=None), dict(ctx=None)):
        assert call(**kw) == 1 and b"null operand" in L.lib().ufnd_last_error()
    for T in (65, 0, -3, 128):
        assert call(T=T) == 1
        msg = L.lib().ufnd_last_error()
        assert f"T={T}".encode() in msg and b"ufnd_attention_bf16" in msg, msg
    for kw in (dict(ldx=H + 4), dict(ldw=H + 2), dict(ldx=H - 8), dict(X=p + 8), dict(W=p + 2), dict(ctx=p + 4)):
        assert call(**kw) == 1 and b"strides must be multiples of 8" in L.lib().ufnd_last_error(), kw
    assert call(b=p + 4) == 1 and b"bias alignment" in L.lib().ufnd_last_error()
    assert call(heads=0) == 1 and call(N=0) == 1
    # the 128-token entries keep refusing what they refused
    assert L.lib().ufnd_qkv_attention_bf16(p, p, p, None, p, 3, 64, 2, H, H, None, None) == 1
    assert b"128-token" in L.lib().ufnd_last_error()
