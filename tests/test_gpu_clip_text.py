"""The CLIP text tower and the semantic analyzer (ultrafnd_git_amd/semantic.py) against the float64 yardsticks of
tests/clip_text_ref.py: the installed transformers.CLIPTextModelWithProjection in float64 (seeded weights, never from_pretrained),
the reference's own head (tests/golden/semantic.npz) and float64 restatements.

Bounds: the causal attention op alone is held elementwise to the bound derived from its roundings (clip_text_ref.causal_attn_ref_bound);
every bf16 stage and the features, on each of the three criteria (max-abs, relative L2, 1 - cosine), to 3 x the bf16-operand mirror's
own error against float64 ON THAT SAME INPUT; fp32-only stages to the rounding bounds written out in clip_text_ref.  Exact
properties (causality, packed = padded, alone = in a batch, run = run) are bit comparisons.  Every test prints its figures before it
asserts; tools/clip_text_errors.py collects them.
"""
import numpy as np
import pytest
import torch

from tests import clip_text_ref as R
from tests import frozen_ops_cases as FO

pytestmark = pytest.mark.gpu
DEV = "cuda"
L77 = 77


def _bf16_dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(torch.bfloat16)


def _bits_host(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


class _Case:
    """A 2-layer encoder per pooling rule with the tests' weights, its HF float64 twin, and per-input reference / mirror results
    computed once and shared."""

    def __init__(self, eos, layers=2):
        from ultrafnd_git_amd.semantic import ClipTextEncoder
        self.eos, self.layers = eos, layers
        enc = ClipTextEncoder(num_hidden_layers=layers, vocab_size=R.VOCAB, eos_token_id=eos)
        enc.load_state_dict(R.case_weights(enc.state_dict()))
        self.sd = enc.state_dict()
        self.enc = enc.to(DEV)
        self.model = R.hf_model(self.sd, layers, eos)
        self._memo = {}

    def ref_mir(self, key, ids, mask):
        if key not in self._memo:
            self._memo[key] = (R.reference(self.model, ids, mask), R.mirror(self.sd, ids, mask, self.layers, self.eos))
        return self._memo[key]


@pytest.fixture(scope="module")
def cases():
    return {eos: _Case(eos) for eos in (R.EOS, 2)}


def _hold(name, got, ref, mir):
    """got within 3 x the mirror's own error of the float64 reference, on each criterion."""
    c, b = R.criteria(got.double().cpu(), ref), R.bounds_from_mirror(mir, ref)
    for k in c:
        print(f"CLIP_TEXT_ERR {name} {k} gpu={c[k]:.3e} bound={b[k]:.3e} ratio_to_mirror={R.BOUND_FACTOR * c[k] / b[k]:.2f}")
    bad = {k: (c[k], b[k]) for k in c if not c[k] <= b[k]}
    assert not bad, (name, bad)


def _hold_abs(name, got, ref, bound):
    """max-abs error of got against ref within `bound` (a rounding bound, absolute)."""
    err = float((torch.as_tensor(got).double().cpu() - torch.as_tensor(ref).double()).abs().max())
    print(f"CLIP_TEXT_ERR {name} max_abs gpu={err:.3e} bound={bound:.3e} ratio_to_bound={err / bound:.2f}")
    assert err <= bound, (name, err, bound)


# ---------------------------------------------------------------------------------------------------------------------
# the causal attention op alone
@pytest.mark.parametrize("L", R.ATTN_LENGTHS)
@pytest.mark.parametrize("B", (1, 3))
def test_causal_attention_op_against_float64(B, L):
    """heads = 4, 8 and 16 (the widths 256, 512 and 1024); the padded and the cu_seqlens form, each without a key mask and with a prefix mask
    (key 0 always kept).  The lengths run past the tower's own 77 to 248: two to four key blocks and query workgroups, every edge from
    both sides.  The bound is the derived one at every length: its nblk = ceil(L / 64) follows the key blocks."""
    for heads in R.ATTN_HEADS:
        _causal_attention_op(B, L, heads)


def _causal_attention_op(B, L, heads):
    from ultrafnd_git_amd import _lib as Lb
    lib = Lb.lib()
    H = heads * 64
    bits = R.attn_inputs(B, L, heads, seed=L)
    qkv = _bf16_dev(bits)
    s = Lb.stream_ptr(torch.device(DEV))
    for mask in (None, R.attn_prefix_mask(B, L)):
        tag = f"attn.B{B}.L{L}.h{heads}.{'prefix' if mask is not None else 'nomask'}"
        mdev = None if mask is None else torch.from_numpy(mask).to(DEV)
        # ---- padded
        ref, bound = R.causal_attn_ref_bound(bits, mask, B, L, heads)
        ctx = torch.full((B * L + 4, H), float("nan"), dtype=torch.bfloat16, device=DEV)      # (four sentinel rows behind the output)
        Lb.check(lib.ufnd_attention_bf16_causal(qkv.data_ptr(), Lb.ptr(mdev), ctx.data_ptr(), B, L, heads, s), "ufnd_attention_bf16_causal")
        torch.cuda.synchronize()
        got = FO.bf16_f32(_bits_host(ctx))
        assert np.isnan(got[B * L:]).all(), (tag, "a row past B L was written")
        ratio = FO.worst_ratio(got[:B * L], ref, bound)
        print(f"CLIP_TEXT_ERR {tag}.padded elementwise gpu={ratio:.3e} bound=1.000e+00 ratio_to_bound={ratio:.2f}")
        assert ratio <= 1.0, (tag, "padded", ratio)
        # ---- cu_seqlens: sample b keeps its first n_b rows (L, about half, 1, ...), packed back to back; keys masked by mask[b][key]
        n = [L, max(1, (L + 1) // 2), 1][:B]
        cu = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        rows = np.concatenate([np.arange(b * L, b * L + n[b]) for b in range(B)])
        cap = B * L
        pk = np.zeros((cap, 3 * H), dtype=np.uint16)
        pk[:len(rows)] = bits[rows]
        refs, bounds = zip(*[R.causal_attn_ref_bound(bits[b * L:b * L + n[b]], None if mask is None else mask[b:b + 1, :n[b]], 1, n[b], heads)
                             for b in range(B)])
        ctx = torch.full((cap, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        Lb.check(lib.ufnd_attention_bf16_causal_varlen(_bf16_dev(pk).data_ptr(), torch.from_numpy(cu).to(DEV).data_ptr(), Lb.ptr(mdev), ctx.data_ptr(), B, L,
                                                       heads, s), "ufnd_attention_bf16_causal_varlen")
        torch.cuda.synchronize()
        got = FO.bf16_f32(_bits_host(ctx))
        ratio = FO.worst_ratio(got[:len(rows)], np.concatenate(refs), np.concatenate(bounds))
        print(f"CLIP_TEXT_ERR {tag}.varlen elementwise gpu={ratio:.3e} bound=1.000e+00 ratio_to_bound={ratio:.2f}")
        assert ratio <= 1.0, (tag, "varlen", ratio)
        assert np.isnan(got[len(rows):]).all(), (tag, "a row past cu[B] was written")


# ---------------------------------------------------------------------------------------------------------------------
# causality, exact
@pytest.fixture(scope="module")
def causal_base(cases):
    ids = R.make_ids((L77 - 1,), L77, seed=77)
    mask = torch.ones_like(ids)
    return ids, mask, cases[R.EOS].enc.last_hidden_state(ids, mask, packed=False).clone()


@pytest.mark.parametrize("j", R.CAUSAL_J)
def test_a_changed_token_never_reaches_an_earlier_row(cases, causal_base, j):
    """Rows < j of last_hidden_state (padded pass, two layers) are the same bits whatever token sits at position j; row j is not.  A
    leak across a tile, wave or key-block edge cannot pass this."""
    ids, mask, base = causal_base
    ids2 = ids.clone()
    ids2[0, j] = 3 + (int(ids[0, j]) - 3 + 101) % (R.VOCAB - 4)
    assert int(ids2[0, j]) != int(ids[0, j])
    got = cases[R.EOS].enc.last_hidden_state(ids2, mask, packed=False)
    assert torch.equal(got[0, :j], base[0, :j]), j
    assert not torch.equal(got[0, j], base[0, j]), j
    assert torch.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------------
# stages against float64
@pytest.mark.parametrize("packed", (False, True), ids=("padded", "packed"))
@pytest.mark.parametrize("batch", (0, 1))
@pytest.mark.parametrize("eos", (R.EOS, 2))
def test_stages_against_float64(cases, eos, batch, packed):
    """B = 5, L = 77, the pooled positions {1, 15, 16, 63, 64, 76} spread over two batches, under both pooling rules: the embeddings
    (fp32 bound), the hidden state after layers 1 and 2 (rows 0 .. e(b), the rows the tower is about), the pooled row, text_embeds and
    the features."""
    c, e_list = cases[eos], R.STAGE_BATCHES[batch]
    ids, mask = R.make_ids(e_list, L77, seed=1), R.prefix_mask(e_list, L77)
    ref, mir = c.ref_mir(("stage", batch), ids, mask)
    live = mask.bool()
    tag = f"stage.eos{eos}.b{batch}.{'packed' if packed else 'padded'}"
    assert c.enc.pooled_positions(ids).tolist() == list(e_list)
    emb = c.enc.last_hidden_state(ids, mask, packed=packed, n_layers=0).cpu()
    _hold_abs(f"{tag}.embed", emb[live], ref["embed"][live], R.FP32_BOUNDS["embed"] * float(ref["embed"][live].abs().max()))
    for k in (1, 2):
        h = c.enc.last_hidden_state(ids, mask, packed=packed, n_layers=k).cpu()
        _hold(f"{tag}.layer{k}", h[live], ref["layers"][k - 1][live], mir["layers"][k - 1][live])
        if packed:
            assert not h[~live].any(), "rows past e(b) are zero in the packed pass"
    _hold(f"{tag}.pooled", c.enc.pooled(ids, mask, packed=packed), ref["pooled"], mir["pooled"])
    _hold(f"{tag}.text_embeds", c.enc.text_embeds(ids, mask, packed=packed), ref["text_embeds"], mir["text_embeds"])
    feat = c.enc(ids, mask, packed=packed)
    _hold(f"{tag}.feature", feat, ref["feature"], mir["feature"])
    # HF's last_hidden_state (final_layer_norm applied), on the pooled rows: the same LayerNorm as the pool kernel's, unrounded
    lhs = c.enc.last_hidden_state(ids, mask, packed=packed).cpu()
    rows = torch.arange(len(e_list)), torch.tensor(e_list)
    _hold(f"{tag}.last_hidden_eos", lhs[rows], ref["pooled"], mir["pooled"])


# ---------------------------------------------------------------------------------------------------------------------
# packed = padded, alone = in a batch, run = run: bit comparisons
def test_packed_pass_is_the_padded_pass_bit_for_bit(cases):
    c = cases[R.EOS]
    e_list = (1, 15, 16, 40, 63, 64, 76)
    ids, mask = R.make_ids(e_list, L77, seed=9), R.prefix_mask(e_list, L77)
    padded = c.enc(ids, mask, packed=False).clone()
    packed = c.enc(ids, mask, packed=True).clone()
    again = c.enc(ids, mask, packed=True).clone()
    alone = torch.cat([c.enc(ids[b:b + 1], mask[b:b + 1], packed=True).clone() for b in range(len(e_list))])
    alone_padded = torch.cat([c.enc(ids[b:b + 1], mask[b:b + 1], packed=False).clone() for b in range(len(e_list))])
    # garbage after e(b): other words, out-of-range ids (clamped by the embedding, never read by the packed pass), and a mask of ones
    junk = ids.clone()
    g = torch.Generator().manual_seed(5)
    for b, e in enumerate(e_list):
        junk[b, e + 1:] = torch.randint(3, R.VOCAB - 1, (L77 - e - 1,), generator=g)
        if e + 2 < L77:
            junk[b, e + 2] = 10 ** 9 if b % 2 else -7
    junk_packed = c.enc(junk, torch.ones_like(junk), packed=True).clone()
    junk_padded = c.enc(junk, torch.ones_like(junk), packed=False).clone()
    res = {"packed_vs_padded": torch.equal(packed, padded), "run_vs_run": torch.equal(packed, again), "alone_vs_batch": torch.equal(alone, packed),
           "alone_padded_vs_batch": torch.equal(alone_padded, padded), "garbage_packed": torch.equal(junk_packed, packed),
           "garbage_padded": torch.equal(junk_padded, padded)}
    print("CLIP_TEXT_BITS " + " ".join(f"{k}={v}" for k, v in res.items()))
    assert all(res.values()), res
    assert torch.isfinite(packed).all() and float((packed.norm(dim=-1) - 1).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# full depth once
def test_full_depth_features_against_float64():
    c = _Case(R.EOS, layers=12)
    ids, mask = R.make_ids(R.FULL_DEPTH_E, L77, seed=12), R.prefix_mask(R.FULL_DEPTH_E, L77)
    ref, mir = c.ref_mir("full", ids, mask)
    _hold("full12.feature", c.enc(ids, mask), ref["feature"], mir["feature"])
    assert torch.equal(c.enc(ids, mask, packed=True).clone(), c.enc(ids, mask, packed=False))


# ---------------------------------------------------------------------------------------------------------------------
# the head
def _small_encoder():
    from ultrafnd_git_amd.semantic import ClipTextEncoder
    return ClipTextEncoder(num_hidden_layers=1, vocab_size=R.VOCAB, eos_token_id=R.EOS)


def _head_check(tag, an, t, i, extra=0.0):
    p = [x.detach().cpu() for x in (an.text_proj[0].weight, an.text_proj[0].bias, an.vision_proj[0].weight, an.vision_proj[0].bias)]
    out = an.head(t.to(DEV), i.to(DEV))
    ref, bound = R.head_ref(t, i, *p), R.head_bounds(t, i, *p)
    for k in ref:
        _hold_abs(f"{tag}.{k}", out[k], ref[k], bound[k] + extra)
    return out


def test_head_reproduces_the_reference_module(golden_dir):
    from ultrafnd_git_amd.semantic import SemanticConfig, SemanticForgeryAnalyzer
    g = np.load(golden_dir / "semantic.npz")
    an = SemanticForgeryAnalyzer(SemanticConfig(proj_dim=128), device=DEV, text_encoder=_small_encoder())
    an.load_state_dict({k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}, strict=True)
    t, i = torch.from_numpy(g["text_feat"]), torch.from_numpy(g["image_feat"])
    out = _head_check("head.golden128", an, t, i)
    # the reference's own fp32 outputs: within our bound plus its own distance from float64 (<= 600 eps, tests/test_clip_text_ref.py)
    b = R.head_bounds(t, i, *[an.state_dict()[k].cpu() for k in ("text_proj.0.weight", "text_proj.0.bias", "vision_proj.0.weight", "vision_proj.0.bias")])
    for k in ("semantic_text", "semantic_image", "semantic_gap"):
        _hold_abs(f"head.reference128.{k}", out[k], torch.from_numpy(g["out/" + k]), b[k] + 600 * R.EPS32)


def test_head_against_float64_at_512_and_from_fusion_shares_storage():
    from ultrafnd_git_amd.fusion import CrossModalTransformer
    from ultrafnd_git_amd.semantic import SemanticForgeryAnalyzer
    fusion = CrossModalTransformer().to(DEV)
    an = SemanticForgeryAnalyzer.from_fusion(fusion, text_encoder=_small_encoder())
    for side in ("text_proj", "vision_proj"):
        for n in ("weight", "bias"):
            assert getattr(getattr(an, side)[0], n).data_ptr() == getattr(getattr(fusion.semantic, side)[0], n).data_ptr(), (side, n)
    assert an.out_dim == 512 and sorted(an.state_dict()) == sorted(k[len("semantic."):] for k in fusion.state_dict() if k.startswith("semantic."))
    g = torch.Generator().manual_seed(3)
    t, i = (torch.nn.functional.normalize(torch.randn(37, 512, generator=g), dim=-1) for _ in range(2))      # 37 rows: three 16-row tiles, the last ragged
    _head_check("head.float64_512", an, t, i)
    with torch.no_grad():      # the shared tensors drive the head: a change made through fusion is seen
        fusion.semantic.text_proj[0].bias.add_(0.25)
    _head_check("head.float64_512_shared", an, t, i)


# ---------------------------------------------------------------------------------------------------------------------
# similarity, and the image side from frames
def test_similarity_against_float64_cosine():
    from ultrafnd_git_amd import _lib as Lb
    g = torch.Generator().manual_seed(4)
    t, i = torch.randn(37, 512, generator=g), 3.0 * torch.randn(37, 512, generator=g)
    i[0], i[1], i[2] = t[0], -2.0 * t[1], t[2] + 0.01 * i[2]      # cosine 1, -1, nearly 1
    sim, conf = torch.empty(37, device=DEV), torch.empty(37, device=DEV)
    td, idv = t.to(DEV), i.to(DEV)
    Lb.check(Lb.lib().ufnd_clip_similarity(td.data_ptr(), idv.data_ptr(), sim.data_ptr(), conf.data_ptr(), 37, 512, Lb.stream_ptr(td.device)),
             "ufnd_clip_similarity")
    cos, conflict = R.similarity_ref(t, i)
    _hold_abs("similarity.cosine", sim, cos, R.FP32_BOUNDS["cosine"])
    _hold_abs("similarity.conflict", conf, conflict, R.FP32_BOUNDS["cosine"] / 2 + 2 * R.EPS32)
    assert abs(float(sim[0]) - 1) < 1e-6 and abs(float(sim[1]) + 1) < 1e-6 and float(conf.min()) >= 0 and float(conf.max()) <= 1


@pytest.mark.parametrize("frames_per_sample", (1, 2))
def test_analyzer_with_frames_and_with_the_text_proxy(frames_per_sample):
    """forward(batch): with `frames`, semantic_image equals l2n(vision_proj(l2n(image_embeds))) -- mean over frames, then l2n, for several
    -- computed in float64 from the GPU's own image_embeds; with ocr ids, the reference's text proxy.  clip_similarity is the cosine of
    the two sides' features."""
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    from ultrafnd_git_amd.semantic import SemanticConfig, SemanticForgeryAnalyzer
    enc = _small_encoder()
    enc.load_state_dict(R.case_weights(enc.state_dict()))
    vis = ClipVisualEncoder(layers=1)
    an = SemanticForgeryAnalyzer(SemanticConfig(proj_dim=128), device=DEV, text_encoder=enc, visual_encoder=vis)
    p = [x.detach().cpu() for x in (an.text_proj[0].weight, an.text_proj[0].bias, an.vision_proj[0].weight, an.vision_proj[0].bias)]
    e_list = (5, 30)
    ids, mask = R.make_ids(e_list, 40, seed=2), R.prefix_mask(e_list, 40)
    ocr, ocr_mask = R.make_ids((12, 3), 24, seed=3), R.prefix_mask((12, 3), 24)
    g = torch.Generator().manual_seed(6)
    frames = torch.randn(2, frames_per_sample, 3, 224, 224, generator=g)
    txt = an.text_encoder(ids, mask).clone().cpu()
    tag = f"analyzer.F{frames_per_sample}"
    # ---- frames
    out = an({"title_ids": ids, "title_mask": mask, "frames": frames if frames_per_sample > 1 else frames[:, 0]})
    ie = an.visual_encoder.image_embeds(frames.view(-1, 3, 224, 224).to(DEV)).double().cpu().view(2, frames_per_sample, 512)
    img = R._l2n(ie)
    if frames_per_sample > 1:
        img = R._l2n(img.mean(dim=1, keepdim=True))
    img = img[:, 0]
    gpu_img = an.visual_encoder(frames.to(DEV)).clone().cpu()
    # l2n in fp32: a 512-term sum, a square root, the division (and the mean over frames): <= (512 + 16) eps of a unit vector's largest entry
    _hold_abs(f"{tag}.image_feature", gpu_img, img, 528 * R.EPS32)
    ref, bound = R.head_ref(txt, gpu_img, *p), R.head_bounds(txt, gpu_img, *p)
    for k in ref:
        _hold_abs(f"{tag}.frames.{k}", out[k], ref[k], bound[k])
    cos, conflict = R.similarity_ref(txt, gpu_img)
    _hold_abs(f"{tag}.frames.clip_similarity", out["clip_similarity"], cos, R.FP32_BOUNDS["cosine"])
    _hold_abs(f"{tag}.frames.semantic_conflict", out["semantic_conflict"], conflict, R.FP32_BOUNDS["cosine"] / 2 + 2 * R.EPS32)
    # ---- the text proxy
    out = an({"title_ids": ids, "title_mask": mask, "ocr_ids": ocr, "ocr_mask": ocr_mask})
    proxy = an.text_encoder(ocr, ocr_mask).clone().cpu()
    ref, bound = R.head_ref(txt, proxy, *p), R.head_bounds(txt, proxy, *p)
    for k in ref:
        _hold_abs(f"{tag}.proxy.{k}", out[k], ref[k], bound[k])
    assert sorted(out) == ["clip_similarity", "semantic_conflict", "semantic_gap", "semantic_image", "semantic_text"]
    with pytest.raises(KeyError):
        an({"title_ids": ids, "title_mask": mask})


# ---------------------------------------------------------------------------------------------------------------------
# the helpers the tower shares with the BERT text encoder: the pack kernels' scan, and LayerNorm inside the pool kernel
@pytest.mark.parametrize("B", (1, 5, 1025, 2049))
def test_pack_scan_is_the_text_pack_scan(B):
    """ufnd_clip_text_pack's cu / row_src against ufnd_text_pack's on the mask l <= e(b), and both against numpy: L = 8, random pooled
    positions that include 0 and L - 1, both pooling rules.  B = 1025 and 2049 give the scan 2 and 3 samples per thread."""
    from ultrafnd_git_amd import _lib as Lb
    lib, Lq, s = Lb.lib(), 8, Lb.stream_ptr(torch.device(DEV))
    rng = np.random.default_rng(B)
    es = [np.array([0]), np.array([Lq - 1])] if B == 1 else [rng.integers(0, Lq, size=B)]
    if B > 1:
        es[0][0], es[0][-1], es[0][B // 2] = 0, Lq - 1, Lq - 1
    for e in es:
        want_cu = np.concatenate([[0], np.cumsum(e + 1)]).astype(np.int32)
        want_src = np.concatenate([b * Lq + np.arange(e[b] + 1) for b in range(B)]).astype(np.int32)
        mask = (np.arange(Lq)[None, :] <= e[:, None]).astype(np.int32)
        cu_t, src_t = torch.full((B + 1,), -1, dtype=torch.int32, device=DEV), torch.full((B * Lq,), -1, dtype=torch.int32, device=DEV)
        Lb.check(lib.ufnd_text_pack(torch.from_numpy(mask).to(DEV).data_ptr(), B, Lq, cu_t.data_ptr(), src_t.data_ptr(), s), "ufnd_text_pack")
        for eos in (R.EOS, 2):      # the first position equal to eos / the first position of the largest id
            ids = rng.integers(3, 40, size=(B, Lq)).astype(np.int64)
            ids[np.arange(B), e] = eos if eos != 2 else 50
            e_c = torch.full((B,), -1, dtype=torch.int32, device=DEV)
            cu_c, src_c = torch.full((B + 1,), -1, dtype=torch.int32, device=DEV), torch.full((B * Lq,), -1, dtype=torch.int32, device=DEV)
            Lb.check(lib.ufnd_clip_text_pack(torch.from_numpy(ids).to(DEV).data_ptr(), B, Lq, eos, e_c.data_ptr(), cu_c.data_ptr(), src_c.data_ptr(), s),
                     "ufnd_clip_text_pack")
            n = int(want_cu[B])
            assert np.array_equal(e_c.cpu().numpy(), e.astype(np.int32)), (B, eos)
            assert np.array_equal(cu_c.cpu().numpy(), want_cu) and np.array_equal(cu_t.cpu().numpy(), want_cu), (B, eos)
            assert np.array_equal(src_c.cpu().numpy()[:n], want_src) and np.array_equal(src_t.cpu().numpy()[:n], want_src), (B, eos)
            assert torch.equal(cu_c, cu_t) and torch.equal(src_c[:n], src_t[:n]), (B, eos)
            assert bool((src_c[n:] == -1).all()) and bool((src_t[n:] == -1).all()), (B, eos)      # nothing written past the live rows


@pytest.mark.parametrize("H", (256, 512, 768, 1024))
def test_pool_is_layernorm_of_the_pooled_rows(H):
    """ufnd_clip_text_pool's bf16 output, bit for bit ufnd_layernorm's on the gathered rows e(b): B = 5, L = 7, fp32 rows with a non-zero
    mean, random e; the padded form (cu NULL: row b L + e[b]) and the packed form (row cu[b + 1] - 1)."""
    from ultrafnd_git_amd import _lib as Lb
    lib, B, Lq, eps, s = Lb.lib(), 5, 7, 1e-5, Lb.stream_ptr(torch.device(DEV))
    g = torch.Generator().manual_seed(H)
    x = (torch.randn(B * Lq, H, generator=g) * 1.7 + 0.9 + torch.randn(B * Lq, 1, generator=g)).to(DEV)
    gamma, beta = (1.0 + 0.3 * torch.randn(H, generator=g)).to(DEV), (0.2 * torch.randn(H, generator=g)).to(DEV)
    e = torch.randint(0, Lq, (B,), generator=g).to(torch.int32)
    e[0], e[1] = 0, Lq - 1
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(e.long() + 1, 0)]).to(torch.int32)
    e_d, cu_d = e.to(DEV), cu.to(DEV)
    for name, cu_arg, rows in (("padded", None, torch.arange(B) * Lq + e.long()), ("packed", cu_d, cu[1:].long() - 1)):
        got = torch.full((B, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        Lb.check(lib.ufnd_clip_text_pool(x.data_ptr(), e_d.data_ptr(), Lb.ptr(cu_arg), gamma.data_ptr(), beta.data_ptr(), got.data_ptr(), B, Lq, H, eps, s),
                 "ufnd_clip_text_pool")
        xg = x[rows.to(DEV)].contiguous()
        want = torch.full((B, H), float("nan"), dtype=torch.bfloat16, device=DEV)
        Lb.check(lib.ufnd_layernorm(xg.data_ptr(), H, gamma.data_ptr(), beta.data_ptr(), want.data_ptr(), None, B, H, eps, s), "ufnd_layernorm")
        torch.cuda.synchronize()
        assert not bool(torch.isnan(want.float()).any())
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (H, name)
