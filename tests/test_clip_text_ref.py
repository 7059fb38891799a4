"""CPU: the CLIP text tower's yardstick, mirror and bounds (tests/clip_text_ref.py) and the host side of ultrafnd_git_amd/semantic.py.

Nothing here touches a GPU: the encoder's state_dict against HF's, the float64 mirror against HF (it IS the yardstick with the bf16
roundings off), the bf16 mirror's error on every input of tests/test_gpu_clip_text.py (the condition that keeps "3 x the mirror" from
being vacuous), the pooled-position rule against both HF branches, and the float64 head against the reference's own module
(tests/golden/semantic.npz).
"""
import numpy as np
import pytest
import torch

from tests import clip_text_ref as R
from ultrafnd_git_amd.semantic import ClipTextEncoder, SemanticConfig, SemanticForgeryAnalyzer

LAYERS = 2


@pytest.fixture(scope="module")
def sd():
    return R.case_weights(ClipTextEncoder(num_hidden_layers=LAYERS, vocab_size=R.VOCAB, eos_token_id=R.EOS).state_dict())


def test_state_dict_names_and_shapes_are_hfs_and_an_hf_state_dict_loads_strictly():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    hf = CLIPTextModelWithProjection(CLIPTextConfig(num_hidden_layers=LAYERS))      # CLIPTextConfig's own defaults otherwise
    enc = ClipTextEncoder(num_hidden_layers=LAYERS)                                 # ... and the encoder's
    hsd, osd = hf.state_dict(), enc.state_dict()
    assert list(hsd) == list(osd)
    assert {k: tuple(v.shape) for k, v in hsd.items()} == {k: tuple(v.shape) for k, v in osd.items()}
    missing, unexpected = enc.load_state_dict(hsd, strict=True)
    assert not missing and not unexpected
    assert all(torch.equal(enc.state_dict()[k], hsd[k]) for k in hsd)
    cfg = hf.config
    assert (enc.vocab, enc.hidden, enc.heads, enc.inter, enc.max_position, enc.proj, enc.eps, enc.eos_token_id) == \
        (cfg.vocab_size, cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size, cfg.max_position_embeddings, cfg.projection_dim,
         cfg.layer_norm_eps, cfg.eos_token_id)
    with pytest.raises(RuntimeError):
        enc.load_state_dict({k: v for k, v in hsd.items() if k != "text_projection.weight"}, strict=True)
    with pytest.raises(ValueError):
        ClipTextEncoder(hidden_act="gelu")


@pytest.mark.parametrize("eos", [R.EOS, 2])
def test_fp32_mode_mirror_is_the_yardstick(sd, eos):
    ids, mask = R.make_ids(R.STAGE_E[:3] + (40,), 77, seed=5), R.prefix_mask(R.STAGE_E[:3] + (40,), 77)
    ref = R.reference(R.hf_model(sd, LAYERS, eos), ids, mask)
    mir = R.mirror(sd, ids, mask, LAYERS, eos, bf16=False)
    live = mask.bool()
    for name in ("embed", "pooled", "text_embeds", "feature"):
        scale = float(ref[name].abs().max())
        assert float((mir[name] - ref[name]).abs().max()) <= R.EPS32 * scale, name
    for k in range(LAYERS):      # rows up to e(b): the rows the tower is about
        scale = float(ref["layers"][k][live].abs().max())
        assert float((mir["layers"][k][live] - ref["layers"][k][live]).abs().max()) <= R.EPS32 * scale, k


@pytest.mark.parametrize("L", sorted(l for l in set(R.ATTN_LENGTHS) - {1} if l <= R.MAX_POS))
def test_bf16_mirror_stays_inside_the_sanity_band_at_every_length(sd, L):
    """L = 1 has one row per sample, which IS its EOS: covered by e = 1 and by the stage inputs below."""
    e_list = sorted({1, L // 2, L - 1} - {0})
    ids, mask = R.make_ids(e_list, L, seed=L), R.prefix_mask(e_list, L)
    ref = R.reference(R.hf_model(sd, LAYERS), ids, mask)
    mir = R.mirror(sd, ids, mask, LAYERS)
    live = mask.bool()
    for name, m, r in [(f"layer{k + 1}", mir["layers"][k][live], ref["layers"][k][live]) for k in range(LAYERS)] + \
                      [(n, mir[n], ref[n]) for n in ("pooled", "text_embeds", "feature")]:
        assert not R.mirror_within_sanity(m, r), (name, R.mirror_within_sanity(m, r))


def test_bf16_mirror_stays_inside_the_sanity_band_at_full_depth():
    sd12 = R.case_weights(ClipTextEncoder(num_hidden_layers=12, vocab_size=R.VOCAB, eos_token_id=R.EOS).state_dict())
    ids, mask = R.make_ids(R.FULL_DEPTH_E, 77, seed=12), R.prefix_mask(R.FULL_DEPTH_E, 77)
    ref = R.reference(R.hf_model(sd12, 12), ids, mask)
    mir = R.mirror(sd12, ids, mask, 12)
    assert not R.mirror_within_sanity(mir["feature"], ref["feature"]), R.mirror_within_sanity(mir["feature"], ref["feature"])


@pytest.mark.parametrize("e_list", R.STAGE_BATCHES)
@pytest.mark.parametrize("eos", [R.EOS, 2])
def test_bf16_mirror_stays_inside_the_sanity_band_on_the_stage_inputs(sd, eos, e_list):
    ids, mask = R.make_ids(e_list, 77, seed=1), R.prefix_mask(e_list, 77)
    ref = R.reference(R.hf_model(sd, LAYERS, eos), ids, mask)
    mir = R.mirror(sd, ids, mask, LAYERS, eos)
    live = mask.bool()
    for name, m, r in [(f"layer{k + 1}", mir["layers"][k][live], ref["layers"][k][live]) for k in range(LAYERS)] + \
                      [(n, mir[n], ref[n]) for n in ("pooled", "text_embeds", "feature")]:
        assert not R.mirror_within_sanity(m, r), (name, R.mirror_within_sanity(m, r))


def _geometry_params():
    from tests import encoder_geometry_cases as G
    return [pytest.param(c, eos, k, id=f"{c.id}-eos{eos}-b{k}") for c in G.CLIP_TEXT_CASES for eos in G.EOS_RULES for k in range(len(c.batches))]


@pytest.mark.parametrize("c,eos,k", _geometry_params())
def test_mirror_at_every_geometry_of_the_table(c, eos, k):
    """tests/encoder_geometry_cases.py: the four widths at L = 77 and the long tower (max_position_embeddings = 248) at L = 128 .. 248.
    With the roundings off the mirror is HF's float64 model at that geometry (the tolerance of test_fp32_mode_mirror_is_the_yardstick);
    with them on it stays inside the sanity band on every input of tests/test_gpu_encoder_geometry.py."""
    from tests import encoder_geometry_cases as G
    ids, mask = G.clip_text_batch(c, k)
    live = mask.bool()
    assert R.pooled_positions(ids, eos).tolist() == list(c.batches[k])
    ref, exact = G.clip_text_ref_mirror(c, eos, k, False)
    for name, got, want in G.stages(ref, exact, live) + [("embed", exact["embed"], ref["embed"])]:
        assert float((got - want).abs().max()) <= R.EPS32 * float(want.abs().max()), name
    _, mir = G.clip_text_ref_mirror(c, eos, k)
    for name, got, want in G.stages(ref, mir, live):
        assert not R.mirror_within_sanity(got, want), (name, R.mirror_within_sanity(got, want))


def test_pooled_position_rule_matches_both_hf_branches():
    """HF pools through these two expressions (modeling_clip.py); R.pooled_positions restates them, and R.reference pools with it --
    so the restatement is held to HF's own pooler_output here, on sequences whose pad token equals EOS and on one whose largest id is
    not its EOS."""
    sd = R.case_weights(ClipTextEncoder(num_hidden_layers=1, vocab_size=R.VOCAB, eos_token_id=R.EOS).state_dict())
    e_list = (1, 7, 20, 31)
    ids = R.make_ids(e_list, 32, seed=3)                     # padded with EOS itself: "first position" decides
    mask = R.prefix_mask(e_list, 32)
    assert R.pooled_positions(ids, R.EOS).tolist() == list(e_list) == R.pooled_positions(ids, 2).tolist()
    other = R.make_ids(e_list, 32, seed=3, eos=7, pad=0)     # EOS = 7 is NOT the largest id: the two rules part
    assert R.pooled_positions(other, 7).tolist() == list(e_list)
    assert R.pooled_positions(other, 2).tolist() != list(e_list)
    assert R.pooled_positions(torch.full((1, 8), 5), 7).tolist() == [0]      # no EOS at all: HF's argmax of zeros
    for eos, batch in ((R.EOS, ids), (2, ids), (7, other), (2, other)):
        m = R.hf_model(sd, 1, eos)
        out = m.text_model(input_ids=batch, attention_mask=mask)
        e = R.pooled_positions(batch, eos)
        assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(len(e_list)), e]), eos


def test_float64_head_reproduces_the_reference_module(golden_dir):
    g = np.load(golden_dir / "semantic.npz")
    p = {k: g["param/" + k] for k in ("text_proj.0.weight", "text_proj.0.bias", "vision_proj.0.weight", "vision_proj.0.bias")}
    assert p["text_proj.0.weight"].shape == (128, 512) and g["text_feat"].shape == (5, 512)
    out = R.head_ref(g["text_feat"], g["image_feat"], *p.values())
    for k, v in out.items():      # the reference ran in fp32: a 512-term sum and a 128-term norm, a few hundred eps at most
        assert float((v - torch.from_numpy(g["out/" + k]).double()).abs().max()) <= 600 * R.EPS32, k
    b = R.head_bounds(g["text_feat"], g["image_feat"], *p.values())
    assert all(0 < v < 2.0 ** -8 for v in b.values()), b      # (worst-case chains, yet below one bf16 rounding of a full-scale component)


def test_analyzer_parameters_are_the_references_and_cpu_calls_raise():
    an = SemanticForgeryAnalyzer(SemanticConfig(proj_dim=128), device="cpu", text_encoder=ClipTextEncoder(num_hidden_layers=1, vocab_size=R.VOCAB))
    assert [k for k, _ in an.named_parameters()] == ["text_proj.0.weight", "text_proj.0.bias", "vision_proj.0.weight", "vision_proj.0.bias"]
    assert list(an.state_dict()) == [k for k, _ in an.named_parameters()]
    assert an.cfg.max_length == 64 and an.out_dim == 128
    from ultrafnd_git_amd._lib import UltrafndHipError
    with pytest.raises(UltrafndHipError):
        an.head(torch.zeros(2, 512), torch.zeros(2, 512))
    ids = R.make_ids((3, 5), 8)
    with pytest.raises(UltrafndHipError):
        an.text_encoder(ids, torch.ones_like(ids))
    with pytest.raises(ValueError):
        an({"title_ids": R.make_ids((3,), 65), "title_mask": torch.ones(1, 65), "ocr_ids": ids, "ocr_mask": torch.ones_like(ids)})
