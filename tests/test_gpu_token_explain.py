"""GPU: token and image-patch attributions -- the encoders' data-gradient passes (encoder_train.TextBackprop / VisualBackprop
.forward_saved / .input_grad), the row kernels around them, explain.input_attribution and ForensicTrainer.explain_inputs -- against
the autograd yardstick of tests/token_explain_ref.py.

Bounds.  A gradient that crossed n bf16 encoder layers agrees with the fp32 autograd to about 2^-9 sqrt(4 n) in relative L2
(tests/test_gpu_encoder_train.py); the bound is 2.5 x that (R.rel_bound: 1.4e-2 at 2 layers, 3.4e-2 at 12), per sample, plus that
file's absolute floor: 2e-3 of the largest per-element scale among the samples, times sqrt(elements).  The signed scores of
`tokens` and `patches` are sums in which the terms cancel, so they are measured in the Cauchy-Schwarz scale of the sum instead of
their own norm: ||got - ref||_2 <= rel sqrt(sum ||g||^2 ||x - base||^2) + floor (R.input_attribution returns the scales).
Logits use the head's criterion of tests/test_gpu_explain.py (relative max error <= 5e-4); `delta`, a difference of two logits, the
same tolerance at the logits' scale.  Every test prints what it measured."""
import ctypes as C

import pytest
import torch

from tests import token_explain_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 5e-4
FLOOR = 2e-3


def _crit(a, r) -> float:
    """tests/test_gpu_explain.py::_crit"""
    a, r = torch.as_tensor(a).double().cpu(), torch.as_tensor(r).double().cpu()
    assert a.shape == r.shape, (a.shape, r.shape)
    scale = max(r.abs().max().item(), r.norm().item() / max(1.0, r.numel() ** 0.5), 1e-9)
    e = (a - r).abs().max().item() / scale
    return float("inf") if e != e else e


def _per_sample(got, ref, scale, rel, what) -> float:
    """Every sample b: ||got_b - ref_b||_2 <= rel scale_b + FLOOR top sqrt(n), top = max_b scale_b / sqrt(n).  Returns the worst
    ||got_b - ref_b|| / scale_b."""
    got, ref = got.double().cpu().flatten(1), ref.double().cpu().flatten(1)
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    scale = scale.double().cpu()
    n = ref.shape[1]
    top = (scale / n ** 0.5).max().item()
    err = (got - ref).norm(dim=1)
    worst = (err / scale.clamp_min(1e-30)).max().item()
    print(f"{what}: worst per-sample error / scale {worst:.3e} (bound {rel:.1e}; floor {FLOOR * top * n ** 0.5:.2e} of scales {scale.min().item():.2e} .. {scale.max().item():.2e})")
    assert (err <= rel * scale + FLOOR * top * n ** 0.5).all(), (what, err.tolist(), scale.tolist())
    return worst


def _text_encoder(layers, seed, vocab=1000):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import BertTextEncoder
    w = E.seeded_weights(E.bert_shapes(layers=layers, vocab=vocab), seed)
    enc = BertTextEncoder(layers=layers, vocab_size=vocab)
    enc.load_state_dict(w)
    return enc.to(DEV), w


def _visual_encoder(layers, seed):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    w = E.seeded_weights(E.vit_shapes(layers=layers), seed)
    enc = ClipVisualEncoder(layers=layers)
    enc.load_state_dict(w)
    return enc.to(DEV), w


def _tokens(B, Lq, seed, vocab=1000):
    from oracle import encoders_ref as E
    ids, mask = E.synthetic_tokens(seed, B, Lq, vocab=vocab, min_len=min(8, Lq))
    if Lq == 77:
        mask[1] = 0
        mask[1, 0] = 1                       # a sample with a single real token
    return ids, mask


# ------------------------------------------------------------------------------------------------ 1. the encoder passes alone
@pytest.mark.parametrize("layers,B,Lq", [(2, 2, 64), (2, 3, 77), (12, 2, 64)])
def test_text_input_grad_vs_autograd(layers, B, Lq):
    from ultrafnd_git_amd.encoder_train import TextBackprop
    enc, w = _text_encoder(layers, 31)
    ids, mask = _tokens(B, Lq, 400 + Lq)
    dfeat = torch.randn(B, 768, generator=torch.Generator().manual_seed(90 + layers))       # (as oracle.encoders_ref.probe_loss seeds it)
    bp = TextBackprop(enc)
    feat = bp.forward_saved(ids, mask).clone()
    ds = bp.input_grad(dfeat.to(DEV)).clone()
    ref_feat, ref = R.text_input_grad(w, ids, mask, dfeat)
    assert (feat.cpu().double() - ref_feat).abs().max().item() <= 1.2e-3
    assert ds.shape == (B * Lq, 768)
    ds3, ref3 = ds.view(B, Lq, 768).cpu(), ref.view(B, Lq, 768)
    assert (ds3[mask == 0] == 0).all(), "masked rows carry exactly no gradient"
    _per_sample(ds3, ref3, ref3.flatten(1).norm(dim=1), R.rel_bound(layers), f"text ds, {layers} layers, B={B} L={Lq} ({B * Lq} rows)")
    again = bp.input_grad(dfeat.to(DEV))
    assert torch.equal(again, ds)


@pytest.mark.parametrize("B,Fr", [(2, 1), (3, 3)])
def test_visual_input_grad_vs_autograd(B, Fr):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoder_train import VisualBackprop
    enc, w = _visual_encoder(2, 32)
    frames = E.synthetic_frames(500 + Fr, B, Fr)
    dfeat = torch.randn(B, 512, generator=torch.Generator().manual_seed(91))
    bp = VisualBackprop(enc)
    feat = bp.forward_saved(frames).clone()
    dfr = bp.input_grad(dfeat.to(DEV))
    ref_feat, ref = R.visual_input_grad(w, frames, dfeat)
    assert (feat.cpu() - ref_feat).abs().max().item() <= 1.5e-3
    assert dfr.shape == frames.shape
    _per_sample(dfr, ref, ref.flatten(1).norm(dim=1), R.rel_bound(2), f"vision dframes, 2 layers, B={B} F={Fr} ({B * Fr * 50} tokens)")
    assert torch.equal(bp.input_grad(dfeat.to(DEV)), dfr)


# ------------------------------------------------------------------------------------------------ 2. the row kernels
def test_unpatchify_is_the_exact_inverse_of_patchify():
    """A panel of distinct integers (exact in fp32) goes to frame layout; ufnd_vit_patchify (bf16 output) brings each of its three
    base-128 digit planes back exactly.  Then pixels = grad * (x - base) bit for bit and the per-patch sums."""
    from ultrafnd_git_amd import _lib as L
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    N, S, p = 2, 224, 32
    P, K = (S // p) ** 2, 3 * p * p
    panel = torch.arange(N * P * K, dtype=torch.float32, device=DEV).view(N * P, K)
    grad = torch.full((N, 3, S, S), float("nan"), device=DEV)
    L.check(lib.ufnd_vit_unpatchify_attribution(panel.data_ptr(), None, None, grad.data_ptr(), None, None, N, S, p, s), "unpatchify")
    assert torch.equal(grad.flatten().sort().values, panel.flatten())
    gi, pi = grad.long(), panel.long()
    for div in (1, 128, 128 * 128):
        back = torch.empty(N * P, K, dtype=torch.bfloat16, device=DEV)
        L.check(lib.ufnd_vit_patchify(((gi // div) % 128).float().contiguous().data_ptr(), back.data_ptr(), N, S, p, s), "ufnd_vit_patchify")
        assert torch.equal(back.float(), ((pi // div) % 128).float()), div
    g = torch.Generator().manual_seed(3)
    small = torch.randn(N * P, K, generator=g).to(DEV)
    x, base = torch.randn(N, 3, S, S, generator=g).to(DEV), torch.randn(N, 3, S, S, generator=g).to(DEV)
    for b in (base, None):
        gr, px = torch.empty(N, 3, S, S, device=DEV), torch.empty(N, 3, S, S, device=DEV)
        ps = torch.empty(N, P, device=DEV)
        L.check(lib.ufnd_vit_unpatchify_attribution(small.data_ptr(), x.data_ptr(), L.ptr(b), gr.data_ptr(), px.data_ptr(), ps.data_ptr(), N, S, p, s),
                "unpatchify")
        want = gr * (x - b) if b is not None else gr * x
        assert torch.equal(px, want)
        ref = R.patch_sums(want.double().cpu()[:, None], p)[:, 0]
        assert (ps.cpu().double() - ref).abs().max().item() <= 1e-5 * want.abs().double().cpu().view(N, -1).sum(1).max().item() / P
        ps2 = torch.empty(N, P, device=DEV)
        L.check(lib.ufnd_vit_unpatchify_attribution(small.data_ptr(), x.data_ptr(), L.ptr(b), None, None, ps2.data_ptr(), N, S, p, s), "unpatchify")
        assert torch.equal(ps2, ps)
    assert lib.ufnd_vit_unpatchify_attribution(small.data_ptr(), None, None, None, px.data_ptr(), None, N, S, p, s) == 1      # pixels need x


@pytest.mark.parametrize("R_,H", [(231, 768), (5, 256)])
def test_token_attribution_kernel(R_, H):
    from ultrafnd_git_amd import _lib as L
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    gen = torch.Generator().manual_seed(R_)
    g, sm, base = (torch.randn(R_, H, generator=gen).to(DEV) for _ in range(3))
    mask = (torch.rand(R_, generator=gen) > 0.3).to(torch.int32).to(DEV)
    score, norm = torch.full((R_,), float("nan"), device=DEV), torch.full((R_,), float("nan"), device=DEV)
    L.check(lib.ufnd_token_attribution(g.data_ptr(), H, sm.data_ptr(), H, base.data_ptr(), H, mask.data_ptr(), R_, H, score.data_ptr(), norm.data_ptr(), s),
            "ufnd_token_attribution")
    m = mask.cpu().double()
    gd, dd = g.cpu().double(), (sm - base).cpu().double()
    assert (score[mask == 0] == 0).all() and (norm[mask == 0] == 0).all()
    scale = (gd.norm(dim=1) * dd.norm(dim=1)).max().item()
    assert ((score.cpu().double() - (gd * dd).sum(1) * m).abs().max().item()) <= 1e-6 * scale
    assert ((norm.cpu().double() - gd.norm(dim=1) * m).abs().max().item()) <= 1e-6 * gd.norm(dim=1).max().item()
    L.check(lib.ufnd_token_attribution(g.data_ptr(), H, sm.data_ptr(), H, base.data_ptr(), H, None, R_, H, score.data_ptr(), norm.data_ptr(), s),
            "ufnd_token_attribution")
    assert ((norm.cpu().double() - gd.norm(dim=1)).abs().max().item()) <= 1e-6 * gd.norm(dim=1).max().item()


def test_path_points_and_path_mean():
    from ultrafnd_git_amd import _lib as L
    from ultrafnd_git_amd.explain import _path_points
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    gen = torch.Generator().manual_seed(4)
    rows, W = 37, 772
    x, base = torch.randn(rows, W, generator=gen).to(DEV), torch.randn(rows, W, generator=gen).to(DEV)
    alphas = [(k + 0.5) / 5 for k in range(5)]
    for b in (base, None):
        pts = _path_points(x, b, alphas, rows, W).view(5, rows, W)
        b0 = b if b is not None else torch.zeros_like(x)
        for k, a in enumerate(alphas):
            want = b0.double() + a * (x.double() - b0.double())
            assert (pts[k].double() - want).abs().max().item() <= 4e-7 * max(1.0, want.abs().max().item())
    assert lib.ufnd_path_points(x.data_ptr(), None, (C.c_float * 65)(), 65, rows, W, pts.data_ptr(), s) == 1
    # UFND_ATTR_PATH_MEAN: the signed sum in step order, one call or two chunks of whole steps: the same bits as adding in order
    G = torch.randn(6 * rows, W, generator=gen).to(DEV)
    want = torch.zeros(rows, W)
    for k in range(6):
        want = want + G[k * rows:(k + 1) * rows].cpu()
    want = (want / 6.0).to(DEV)          # (divided on the host: an IEEE division, as the kernel's)
    one, two = torch.full((rows, W), float("nan"), device=DEV), torch.full((rows, W), float("nan"), device=DEV)
    L.check(lib.ufnd_attribution_reduce(L.ATTR_PATH_MEAN, G.data_ptr(), W, None, 0, rows, W, 6, 0, 6, one.data_ptr(), W, None, None, s), "path mean")
    L.check(lib.ufnd_attribution_reduce(L.ATTR_PATH_MEAN, G.data_ptr(), W, None, 0, rows, W, 4, 0, 0, two.data_ptr(), W, None, None, s), "path mean")
    L.check(lib.ufnd_attribution_reduce(L.ATTR_PATH_MEAN, G[4 * rows:].data_ptr(), W, None, 0, rows, W, 2, 1, 6, two.data_ptr(), W, None, None, s), "path mean")
    assert torch.equal(one, want) and torch.equal(two, want)
    assert (one < 0).any()                   # signed: not the smooth-grad mode
    sm = torch.empty(rows, W, device=DEV)
    L.check(lib.ufnd_attribution_reduce(L.ATTR_SMOOTHGRAD, G.data_ptr(), W, None, 0, rows, W, 6, 0, 6, sm.data_ptr(), W, None, None, s), "smooth-grad")
    assert (sm >= 0).all() and not torch.equal(sm, one)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _head(use_gnn=True, seed=1234):
    from oracle import tier_a as O
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.fusion import CrossModalTransformer
    fus_sd, clf_sd = O.seeded_params(seed, use_gnn=use_gnn)
    fusion = CrossModalTransformer("configs/model_configs/fusion.yaml" if use_gnn else "configs/model_configs/fusion_nognn.yaml")
    clf = DeepTruthClassifier()
    fusion.load_state_dict(fus_sd); clf.load_state_dict(clf_sd)
    return fusion.to(DEV).eval(), clf.to(DEV).eval(), {k: v.double() for k, v in fus_sd.items()}, {k: v.double() for k, v in clf_sd.items()}


def _batch(B, Lq, Fr, seed, use_gnn=True):
    from oracle import encoders_ref as E
    from oracle import tier_a as O
    batch = dict(O.seeded_batch(seed, B))
    del batch["text_features"], batch["visual_features"]
    if not use_gnn:
        del batch["gnn_feat"]
    ids, mask = _tokens(B, Lq, seed + 1)
    batch.update({"input_ids": ids, "attention_mask": mask, "frames": E.synthetic_frames(seed + 2, B, Fr)})
    return batch, {k: v.to(DEV) for k, v in batch.items()}


_CASES = {}


def _case(B, Lq, Fr, use_gnn):
    """(modules, encoders, weights, batches) of a geometry, built once per session and left unchanged."""
    key = (B, Lq, Fr, use_gnn)
    if key not in _CASES:
        tenc, wt = _text_encoder(2, 33)
        venc, wv = _visual_encoder(2, 34)
        _CASES[key] = (_head(use_gnn), (tenc, venc), (wt, wv), _batch(B, Lq, Fr, 600 + B + Lq, use_gnn))
    return _CASES[key]


def _check(out, ref, what):
    assert set(out) == set(ref) - {"token_scale", "patch_scale"}, (sorted(out), sorted(ref))
    le = _crit(out["logits"], ref["logits"])
    print(f"{what}: logits {le:.3e} (<= {LOGIT_TOL:.0e})")
    assert le <= LOGIT_TOL
    wt = _per_sample(out["tokens"], ref["tokens"], ref["token_scale"], R.rel_bound(2), what + ", tokens")
    wp = _per_sample(out["patches"], ref["patches"], ref["patch_scale"], R.rel_bound(2), what + ", patches")
    _per_sample(out["token_grad_norm"], ref["token_grad_norm"], ref["token_grad_norm"].norm(dim=1), R.rel_bound(2), what + ", token_grad_norm")
    # pixels: bounded in the patches' scale (||g o x|| <= ||g|| ||x|| patch by patch); against their own norm the error is only
    # printed -- the head's gradient at bf16-computed features loses its radial part in the L2 normalisations, and what remains
    # carries the features' error amplified
    px = out["pixels"].double().cpu()
    pe = ((px - ref["pixels"]).flatten(1).norm(dim=1) / ref["pixels"].flatten(1).norm(dim=1)).max().item()
    print(f"{what}, pixels: worst per-sample relative L2 against their own norm {pe:.3e}")
    _per_sample(px, ref["pixels"], ref["patch_scale"], R.rel_bound(2), what + ", pixels")
    assert (R.patch_sums(px, 32) - out["patches"].double().cpu()).abs().max().item() <= 1e-5 * px.abs().flatten(1).sum(1).max().item() / 49
    return wt, wp


@pytest.mark.parametrize("use_gnn", [True, False])
@pytest.mark.parametrize("B,Lq,Fr", [(2, 32, 1), (3, 77, 2)])
def test_grad_x_input_vs_autograd(B, Lq, Fr, use_gnn):
    from ultrafnd_git_amd.explain import input_attribution
    (fusion, clf, fus, cl), (tenc, venc), (wt, wv), (batch, gb) = _case(B, Lq, Fr, use_gnn)
    for c in (1, 0):
        out = input_attribution(fusion, clf, tenc, venc, gb, class_idx=c)
        ref = R.input_attribution(fus, cl, wt, wv, batch, class_idx=c)
        assert out["tokens"].shape == (B, Lq) and out["patches"].shape == (B, Fr, 49) and out["pixels"].shape == (B, Fr, 3, 224, 224)
        assert (out["tokens"].cpu()[batch["attention_mask"] == 0] == 0).all() and (out["token_grad_norm"].cpu()[batch["attention_mask"] == 0] == 0).all()
        _check(out, ref, f"grad_x_input B={B} L={Lq} F={Fr} gnn={use_gnn} class {c}")


def test_integrated_gradients_vs_autograd_in_one_and_two_chunks():
    from ultrafnd_git_amd.explain import input_attribution
    B, Lq, Fr = 2, 32, 1
    (fusion, clf, fus, cl), (tenc, venc), (wt, wv), (batch, gb) = _case(B, Lq, Fr, True)
    two = input_attribution(fusion, clf, tenc, venc, gb, method="integrated_gradients", steps=4, rows_per_pass=2 * B * Lq)
    ref = R.input_attribution(fus, cl, wt, wv, batch, method="integrated_gradients", steps=4)
    _check(two, ref, "integrated_gradients, 4 steps in two chunks")
    # delta is a difference of two logits: its error is measured where the logits' is, at the logits' scale (against its own size --
    # 2e-3 here, what is left of logits of 0.1 .. 1 after the subtraction -- a bf16 encoder pass cannot hold 5e-4: measured 5.4e-3)
    lscale = ref["logits"].abs().max().item()
    de = (two["delta"].double().cpu() - ref["delta"]).abs().max().item() / lscale
    print(f"delta {two['delta'].tolist()} (yardstick {ref['delta'].tolist()}): {de:.3e} of the logits' scale {lscale:.3f} (<= {LOGIT_TOL:.0e}); "
          f"against its own scale {_crit(two['delta'], ref['delta']):.3e}")
    one = input_attribution(fusion, clf, tenc, venc, gb, method="integrated_gradients", steps=4)
    _per_sample(one["tokens"], two["tokens"], ref["token_scale"], R.rel_bound(2), "one chunk vs two, tokens")
    _per_sample(one["patches"], two["patches"], ref["patch_scale"], R.rel_bound(2), "one chunk vs two, patches")
    again = input_attribution(fusion, clf, tenc, venc, gb, method="integrated_gradients", steps=4, rows_per_pass=2 * B * Lq)
    assert all(torch.equal(again[k], two[k]) for k in two)
    gx = input_attribution(fusion, clf, tenc, venc, gb)
    gx2 = input_attribution(fusion, clf, tenc, venc, gb)
    assert all(torch.equal(gx[k], gx2[k]) for k in gx) and "delta" not in gx
    assert de <= LOGIT_TOL
    with pytest.raises(ValueError):
        input_attribution(fusion, clf, tenc, venc, gb, class_idx=2)
    with pytest.raises(ValueError):
        input_attribution(fusion, clf, tenc, venc, gb, method="lime")
    with pytest.raises(ValueError):
        input_attribution(fusion, clf, tenc, venc, gb, method="integrated_gradients", steps=0)


# ------------------------------------------------------------------------------------------------ 4. nothing of the encoders moves
def test_frozen_encoders_are_left_as_found():
    from ultrafnd_git_amd.explain import input_attribution
    (fusion, clf, _, _), (tenc, venc), _, (batch, gb) = _case(2, 32, 1, True)
    mask = gb["attention_mask"].to(torch.int32)
    f_t, f_v = tenc(gb["input_ids"], mask).clone(), venc(gb["frames"]).clone()
    state = [(e.weights_version, e._packed, {k: v.clone() for k, v in e._w.items()}) for e in (tenc, venc)]
    assert all(p is not None for _, p, _ in state)
    input_attribution(fusion, clf, tenc, venc, gb)
    input_attribution(fusion, clf, tenc, venc, gb, method="integrated_gradients", steps=2)
    for e, (ver, packed, w) in zip((tenc, venc), state):
        assert e.weights_version == ver and e._packed is packed
        assert all(torch.equal(e._w[k], v) for k, v in w.items())
    assert torch.equal(tenc(gb["input_ids"], mask), f_t) and torch.equal(venc(gb["frames"]), f_v)


def test_bound_encoders_keep_their_gradients_and_a_pending_backward():
    from oracle import encoders_ref as E
    from tests.test_gpu_encoder_train import _standalone
    from ultrafnd_git_amd.encoder_train import TextBackprop, VisualBackprop
    tenc, _ = _text_encoder(2, 35)
    venc, _ = _visual_encoder(2, 36)
    ids, mask = _tokens(3, 40, 700)
    frames = E.synthetic_frames(701, 3, 2)
    gen = torch.Generator().manual_seed(702)
    dt, dv = torch.randn(3, 768, generator=gen).to(DEV), torch.randn(3, 512, generator=gen).to(DEV)
    for bp_cls, enc, fwd, d in ((TextBackprop, tenc, (ids, mask), dt), (VisualBackprop, venc, (frames,), dv)):
        bp, arena = _standalone(bp_cls, enc)
        bp.forward_train(*fwd)
        bp.backward(d)
        torch.cuda.synchronize()
        plain = arena.grad.clone()
        arena.grad.fill_(float("nan"))
        params = arena.data.clone()
        bp.forward_train(*fwd)                               # ... waits for its backward while the explanation runs
        bp.forward_saved(*fwd)                               # the same shape: buffers of its own
        g1 = bp.input_grad(2 * d).clone()
        torch.cuda.synchronize()
        assert torch.isnan(arena.grad).all() and torch.equal(arena.data, params) and torch.isfinite(g1).all()
        bp.backward(d)
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(arena.grad, nan=-7.0), torch.nan_to_num(plain, nan=-7.0)), bp_cls.__name__
        # a frozen copy of the same weights gives the same bits: the operand copies are cast the same way
        fz = bp_cls(enc.__class__(layers=2, **({"vocab_size": 1000} if bp_cls is TextBackprop else {})).to(DEV))
        fz.enc.load_state_dict(enc.state_dict())
        fz.forward_saved(*fwd)
        assert torch.equal(fz.input_grad(2 * d), g1), bp_cls.__name__


@pytest.mark.parametrize("overlap", [True, False])
def test_backward_and_input_grad_are_one_chain_bit_for_bit(overlap):
    """backward() and input_grad() walk the same chain, so at dropout 0 its two modes give the same data gradients to the bit: text
    the raw embedding sums' (`ds`), vision the patch embedding's output's (`dpe`) -- and the mode without parameter gradients leaves
    the arena's gradient buffer as backward() wrote it.  Text 3 x 77 (231 rows, not a multiple of 64; sample 1 has a single real
    token), vision 2 x 2 frames (200 token rows, 4 CLS rows): row padding, masked rows and the CLS-only gradient all occur."""
    from oracle import encoders_ref as E
    from tests.test_gpu_encoder_train import _standalone
    from ultrafnd_git_amd.encoder_train import TextBackprop, VisualBackprop
    tenc, _ = _text_encoder(2, 37)
    venc, _ = _visual_encoder(2, 38)
    ids, mask = _tokens(3, 77, 710)
    frames = E.synthetic_frames(711, 2, 2)
    gen = torch.Generator().manual_seed(712)
    dt, dv = torch.randn(3, 768, generator=gen).to(DEV), torch.randn(2, 512, generator=gen).to(DEV)
    for bp_cls, enc, fwd, d, key in ((TextBackprop, tenc, (ids, mask), dt, "ds"), (VisualBackprop, venc, (frames,), dv, "dpe")):
        bp, arena = _standalone(bp_cls, enc)
        bp.overlap_wgrad = overlap
        bp.forward_train(*fwd)
        bp.backward(d)
        torch.cuda.synchronize()
        full, grads = bp.saved["sv"][key].clone(), arena.grad.clone()
        assert torch.isfinite(full).all() and full.abs().max().item() > 0
        bp.forward_saved(*fwd)
        got = bp.input_grad(d)
        torch.cuda.synchronize()
        data = got if key == "ds" else bp.xsaved["sv"][key]
        assert data.data_ptr() != bp.saved["sv"][key].data_ptr()
        assert torch.equal(data, full), (bp_cls.__name__, key, overlap)
        assert torch.equal(arena.grad.view(torch.int32), grads.view(torch.int32)), bp_cls.__name__       # (as bits: the padding is NaN)


# ------------------------------------------------------------------------------------------------ 5. the trainer
def _inline_trainer(tmp_path, train_encoders, use_graph):
    from oracle import tier_a as O
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    tenc, _ = _text_encoder(2, 11, vocab=500)
    venc, _ = _visual_encoder(2, 12)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=4, device=DEV, use_graph=use_graph, encode_inline=True,
                      train_encoders=train_encoders)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(16, seed=1), text_encoder=tenc, visual_encoder=venc)
    fus_sd, clf_sd = O.seeded_params(1234)
    tr.fusion.load_state_dict(fus_sd); tr.clf.load_state_dict(clf_sd)
    tr.fusion.train(); tr.clf.train()
    return tr


def _inline_batches(n, B=4, Lq=32):
    from oracle import encoders_ref as E
    from oracle import tier_a as O
    out = []
    for i in range(n):
        ids, mask = E.synthetic_tokens(13 + i, B, Lq, vocab=500, min_len=8)
        gb = {k: v.to(DEV) for k, v in O.seeded_batch(15 + i, B).items()}
        gb.update({"input_ids": ids.to(DEV), "attention_mask": mask.to(torch.int32).to(DEV), "frames": E.synthetic_frames(14 + i, B, 1).to(DEV)})
        out.append(gb)
    return out


@pytest.mark.parametrize("train_encoders,use_graph", [(False, True), (True, False)])
def test_explain_inputs_between_train_steps_changes_nothing(tmp_path, train_encoders, use_graph):
    batches = _inline_batches(3)
    res = []
    for explain in (False, True):
        torch.manual_seed(5)
        tr = _inline_trainer(tmp_path, train_encoders, use_graph)
        losses = []
        for step, gb in enumerate(batches):
            out = tr.train_step(gb)
            losses.append(float(out["loss"].cpu()))
            if explain and step < 2:
                e = tr.explain_inputs(gb, method="grad_x_input" if step == 0 else "integrated_gradients", steps=2)
                assert e["tokens"].shape == (4, 32) and e["patches"].shape == (4, 1, 49) and torch.isfinite(e["tokens"]).all()
                assert tr.fusion.training and tr.clf.training
                with pytest.raises(NotImplementedError, match="encoder-fed"):
                    tr.explain()
        res.append((losses, out["logits"].clone(), tr.arena.data.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_explain_inputs_needs_an_encoder_fed_trainer(tmp_path):
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=4, device=DEV, use_graph=False)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(16, seed=3))
    with pytest.raises(ValueError, match="encode_inline"):
        tr.explain_inputs(_inline_batches(1)[0])
