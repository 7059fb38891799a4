"""CPU: the four frozen encoders refuse, at construction and by argument name, every geometry their kernels are not built for
(DESIGN.md's geometry table) -- instead of constructing and failing at the first launch with a C-ABI message.  And every geometry of
the table constructs, loads its own state_dict strictly and reports the geometry it was given."""
import pytest

from tests import encoder_geometry_cases as G
from ultrafnd_git_amd.affective import RobertaEmotionClassifier
from ultrafnd_git_amd.encoders import MAX_PROJECTION, SUPPORTED_HIDDEN, BertTextEncoder, ClipVisualEncoder
from ultrafnd_git_amd.semantic import ClipTextEncoder

SMALL = dict(vocab_size=64)
# per class: the constructor, its names for (layers, hidden, heads, intermediate, projection_dim or None), small fixed arguments
CLASSES = {
    "bert": (BertTextEncoder, ("layers", "hidden", "heads", "intermediate", None), dict(vocab_size=64, max_position=16)),
    "roberta": (RobertaEmotionClassifier, ("num_hidden_layers", "hidden_size", "num_attention_heads", "intermediate_size", None),
                dict(vocab_size=64, max_position_embeddings=16)),
    "vit": (ClipVisualEncoder, ("layers", "hidden", "heads", "intermediate", "projection_dim"), dict(image=64)),
    "clip_text": (ClipTextEncoder, ("num_hidden_layers", "hidden_size", "num_attention_heads", "intermediate_size", "projection_dim"),
                  dict(vocab_size=64, max_position_embeddings=16)),
}


def _build(name, hidden=256, heads=4, intermediate=256, projection_dim=64, **more):
    cls, (n_layers, n_hidden, n_heads, n_inter, n_proj), fixed = CLASSES[name]
    kw = {n_layers: 1, n_hidden: hidden, n_heads: heads, n_inter: intermediate, **fixed, **more}
    if n_proj is not None:
        kw[n_proj] = projection_dim
    return cls(**kw)


def test_the_supported_values_are_the_kernels():
    assert SUPPORTED_HIDDEN == (256, 512, 768, 1024) and MAX_PROJECTION == 1024


@pytest.mark.parametrize("name", list(CLASSES))
def test_a_width_without_row_kernels_is_refused_by_name(name):
    n_hidden = CLASSES[name][1][1]
    for hidden in (192, 128, 320, 384, 640, 1280, 2048):
        with pytest.raises(ValueError, match=rf"{n_hidden}={hidden}: one of \(256, 512, 768, 1024\)"):
            _build(name, hidden=hidden, heads=hidden // 64)
    for hidden in SUPPORTED_HIDDEN:
        enc = _build(name, hidden=hidden, heads=hidden // 64)
        assert (enc.hidden, enc.heads) == (hidden, hidden // 64)


@pytest.mark.parametrize("name", list(CLASSES))
def test_a_head_count_that_is_not_hidden_over_64_is_refused_by_name(name):
    n_heads = CLASSES[name][1][2]
    for hidden, heads in ((256, 8), (768, 8), (512, 4), (1024, 8)):
        with pytest.raises(ValueError, match=rf"{n_heads}={heads}: .*head_dim must be 64"):
            _build(name, hidden=hidden, heads=heads)


@pytest.mark.parametrize("name", list(CLASSES))
def test_an_intermediate_size_that_is_no_multiple_of_64_is_refused_by_name(name):
    n_inter = CLASSES[name][1][3]
    for inter in (0, 32, 100, 1000, 3072 + 32):
        with pytest.raises(ValueError, match=rf"{n_inter}={inter}: a positive multiple of 64"):
            _build(name, intermediate=inter)
    assert _build(name, intermediate=640).inter == 640


@pytest.mark.parametrize("name", ("vit", "clip_text"))
def test_a_projection_dim_off_the_grid_or_above_1024_is_refused_by_name(name):
    for proj in (0, 32, 100, 500, 1088, 2048):
        with pytest.raises(ValueError, match=rf"projection_dim={proj}: a multiple of 64 from 64 to 1024"):
            _build(name, projection_dim=proj)
    for proj in (64, 192, 1024):
        assert _build(name, projection_dim=proj).proj == proj


def test_vit_patch_and_image_are_refused_by_name():
    # a patch that is no multiple of 8: its rows are no whole 8-pixel runs, and the patch GEMM's K = 3 patch^2 (48, 432, 300) is no
    # multiple of 64 either -- with patch % 8 == 0, K = 192 (patch / 8)^2 always is
    for patch, image in ((4, 32), (12, 48), (10, 40), (0, 32), (-8, 32)):
        with pytest.raises(ValueError, match=rf"patch={patch}: a positive multiple of 8"):
            _build("vit", patch=patch, image=image)
    for patch, image in ((32, 224 + 16), (16, 40), (32, 16), (8, 0)):
        with pytest.raises(ValueError, match=rf"image={image}: a positive multiple of patch={patch}"):
            _build("vit", patch=patch, image=image)
    for patch in (8, 16, 24, 32):
        enc = _build("vit", patch=patch, image=4 * patch)
        assert (3 * patch * patch) % 64 == 0 and enc.n_patches == 16


def test_every_geometry_of_the_table_constructs_and_round_trips_its_state_dict():
    for c in G.BERT_CASES + G.ROBERTA_CASES:
        enc = G.text_encoder(c)
        assert (enc.hidden, enc.heads, enc.inter, enc.layers) == (c.hidden, c.heads, c.inter, G.LAYERS)
        assert enc.load_state_dict(enc.state_dict(), strict=True)[0] == []
    for c in G.VIT_CASES:
        enc = G.vit_encoder(c)
        assert (enc.hidden, enc.heads, enc.inter, enc.patch, enc.image, enc.proj, enc.n_patches + 1) == \
            (c.hidden, c.heads, c.inter, c.patch, c.image, c.proj, c.tokens)
    for c in G.CLIP_TEXT_CASES:
        enc = G.clip_text_encoder(c, G.EOS_RULES[0])
        assert (enc.hidden, enc.heads, enc.inter, enc.proj, enc.max_position) == (c.hidden, c.heads, c.inter, c.proj, c.max_pos)
