"""CPU: the ViT's yardstick and mirror (tests/vit_ref.py) at every geometry of tests/encoder_geometry_cases.py.

Nothing here touches a GPU: the float64 yardstick (oracle/encoders_ref on float64 weights) against the installed
transformers.CLIPVisionModelWithProjection in float64 at two of the new geometries; the mirror with its roundings off against the
yardstick, in each of the three forms; and the bf16 mirror's error on every input of tests/test_gpu_encoder_geometry.py, in the form
the encoder takes there (the condition that keeps "3 x the mirror" from being vacuous)."""
import pytest
import torch

from tests import encoder_geometry_cases as G
from tests import vit_ref as R

CASES = [pytest.param(c, B, Fr, id=f"{c.id}-B{B}F{Fr}") for c in G.VIT_CASES for B, Fr in G.VIT_BATCHES]


@pytest.mark.parametrize("c", G.VIT_HF_PINS, ids=lambda c: c.id)
def test_the_float64_yardstick_is_hfs_model(c):
    """(the tolerance of tests/test_clip_text_ref.py, the other tower of the same HF model: one fp32 unit roundoff of the stage's scale)"""
    sd, frames = G.vit_weights(c.hidden, c.heads, c.inter, c.patch, c.image, c.proj), G.vit_frames(c, 2, 2)
    enc = G.vit_encoder(c)
    hf = R.hf_model(sd, G.LAYERS, c.hidden, c.heads, c.inter, c.patch, c.image, c.proj)
    want = {k: tuple(v.shape) for k, v in hf.state_dict().items() if not k.endswith("position_ids")}
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == want      # the encoder's names and shapes are HF's at this geometry
    ref, got = R.hf_reference(hf, frames), R.reference(sd, frames, c.heads)
    for name in ("embed", "pooled", "image_embeds", "feature"):
        assert float((got[name] - ref[name]).abs().max()) <= R.EPS32 * float(ref[name].abs().max()), name
    for a, b in zip(got["layers"], ref["layers"]):
        assert float((a - b).abs().max()) <= R.EPS32 * float(b.abs().max())


@pytest.mark.parametrize("c,B,Fr", CASES)
def test_mirror_without_rounding_is_the_yardstick_and_with_it_stays_inside_the_sanity_band(c, B, Fr):
    form = G.form_of(G.vit_encoder(c), B, Fr)["form"]
    assert form in R.FORMS
    ref, exact = G.vit_ref_mirror(c, B, Fr, form, False)
    for name, got, want in G.stages(ref, exact) + [("embed", exact["embed"], ref["embed"])]:
        assert torch.allclose(got, want, rtol=0, atol=1e-11), (form, name)
    _, mir = G.vit_ref_mirror(c, B, Fr, form)
    for name, got, want in G.stages(ref, mir) + [("embed", mir["embed"], ref["embed"])]:      # (the patch GEMM rounds its operands: "embed" too)
        assert not R.mirror_within_sanity(got, want), (form, name, R.mirror_within_sanity(got, want))


def test_the_three_forms_differ_and_each_is_exact_without_rounding():
    c = G.VIT_CASES[2]
    assert (c.hidden, c.tokens) == (768, 50)
    ref, _ = G.vit_ref_mirror(c, 3, 1, "unfolded", False)
    feats = {}
    for form in R.FORMS:
        _, exact = G.vit_ref_mirror(c, 3, 1, form, False)
        assert torch.allclose(exact["feature"], ref["feature"], rtol=0, atol=1e-11), form
        feats[form] = G.vit_ref_mirror(c, 3, 1, form)[1]["feature"]
    assert not torch.equal(feats["folded-bf16"], feats["folded-fp32"]) and not torch.equal(feats["folded-fp32"], feats["unfolded"])
