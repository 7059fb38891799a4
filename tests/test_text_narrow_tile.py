"""CPU: which GEMM tile the frozen text encoder names for its out-projection and FFN2 (BertTextEncoder.text_narrow_tile): tile 2
(256x128) on the live-row launches of a packed L = 128 pass of at least 8,192 capacity rows, the library's own choice everywhere else.
Nothing here launches a kernel: the rule is a function of the pass's form and shape alone."""
import ctypes as C

import pytest

from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder

LIVE = 0x1000      # stands for the device address of a live row count: _tile_for only asks whether there is one


@pytest.fixture(scope="module")
def tenc():
    return BertTextEncoder(layers=1, vocab_size=64, max_position=128)


def _chosen(enc, packed, B, Lq, which, m_live=LIVE):
    enc._live_tiles = enc.live_tiles(packed, B, Lq)      # (what _pass does before its first launch)
    return enc._tile_for(which, m_live)


def test_default_is_tile_2_on_the_packed_pass_from_8192_rows(tenc):
    assert tenc.text_narrow_tile == 2 and tenc.text_narrow_min_rows == 8192
    for B in (64, 128, 512):                             # 8,192, 16,384 (the bench's lookahead 4) and 65,536 capacity rows
        assert tenc.live_tiles(True, B, 128) == {"out": 2, "ffn2": 2}
        assert [_chosen(tenc, True, B, 128, w) for w in ("qkv", "out", "ffn1", "ffn2")] == [-1, 2, -1, 2]


def test_every_other_pass_keeps_the_librarys_choice(tenc):
    for packed, B, Lq in ((True, 32, 128),               # lookahead 1: 4,096 capacity rows
                          (True, 63, 128),               # one sample below the threshold
                          (False, 128, 128),             # the padded pass: no live-row entries
                          (True, 128, 64), (True, 64, 256), (True, 32, 512)):      # other lengths, 8,192 rows or more
        assert tenc.live_tiles(packed, B, Lq) == {}
        assert [_chosen(tenc, packed, B, Lq, w) for w in ("qkv", "out", "ffn1", "ffn2")] == [-1] * 4


def test_another_width_keeps_the_librarys_choice():
    """the rule was measured at N = 768; a narrower encoder is left alone (N = 256, the narrowest width with row kernels: a width
    without them no longer constructs, tests/test_encoder_geometry_args.py)"""
    enc = BertTextEncoder(layers=1, hidden=256, heads=4, intermediate=1024, vocab_size=64, max_position=128)
    assert enc.live_tiles(True, 128, 128) == {} and _chosen(enc, True, 128, 128, "ffn2") == -1


def test_a_launch_without_a_live_count_is_not_retiled(tenc):
    """the last layer's class-row tail of a packed pass runs capacity-sized launches over its own few rows"""
    assert _chosen(tenc, True, 128, 128, "out", m_live=None) == -1 and _chosen(tenc, True, 128, 128, "ffn2", m_live=None) == -1


def test_the_attribute_restores_tile_22():
    enc = BertTextEncoder(layers=1, vocab_size=64, max_position=128)
    enc.text_narrow_tile = 22
    assert [_chosen(enc, True, 128, 128, w) for w in ("out", "ffn2")] == [22, 22]
    assert _chosen(enc, True, 32, 128, "out") == -1


def test_an_explicit_tiles_entry_wins():
    enc = BertTextEncoder(layers=1, vocab_size=64, max_position=128)
    enc.tiles = {"out": 16, "qkv": 22}
    assert [_chosen(enc, True, 128, 128, w) for w in ("qkv", "out", "ffn1", "ffn2")] == [22, 16, -1, 2]
    assert [_chosen(enc, True, 32, 128, w) for w in ("qkv", "out", "ffn1", "ffn2")] == [22, 16, -1, -1]
    assert _chosen(enc, True, 128, 128, "out", m_live=None) == 16


def test_the_vit_has_no_such_rule():
    venc = ClipVisualEncoder(layers=1)
    assert not hasattr(venc, "text_narrow_tile") and venc._live_tiles == {}
    assert [venc._tile_for(w, m) for w in ("qkv", "out", "ffn1", "ffn2") for m in (None, LIVE)] == [-1] * 8


def test_stat_parts_and_the_two_tiles():
    """Statistics stay N / 32 = 24 partials per row at every capacity, and tile 2 writes the same count: buffers sized with
    ufnd_gemm_bf16_stat_parts remain right whichever of the two tiles a launch names."""
    from ultrafnd_git_amd import _lib as L
    for M in (4096, 8192, 16384, 65536):
        assert L.lib().ufnd_gemm_bf16_stat_parts(M, 768, 768) == 24 and L.lib().ufnd_gemm_bf16_stat_parts(M, 768, 3072) == 24
    from tests.test_gemm_bf16_cases import plan_args
    from tests.test_gpu_gemm_narrow_tile import case
    from tools import _diaglib as D
    for t, dims, n_tiles in ((2, (256, 128), 6), (22, (256, 192), 4)):
        bm, bn, ln = C.c_int(), C.c_int(), C.c_int()
        assert L.lib().ufnd_gemm_bf16_tile_info(t, C.byref(bm), C.byref(bn), C.byref(ln)) == 1 and (bm.value, bn.value, ln.value) == (*dims, 1)
        for K in (768, 3072):      # the library's own checks and stat_parts_for, for a residual-through-LayerNorm launch that names the tile
            c = case("rln-stats", t, 16384, 768, K)
            rc, p, err = D.gemm_bf16_plan(c.entry, **plan_args(c))
            assert rc == 0 and (p["tile"], p["m_tiles"], p["n_tiles"], p["stat_parts"], p["xcd_cols"]) == (t, 64, n_tiles, 24, 1), (t, K, p, err)
    # the 2-slot W ring variant of tile 2 is sweep material of the diagnostics library, not a tile the product library can be asked for
    rc, p, _ = D.gemm_bf16_plan("tile", tile=30)
    assert rc == 0 and (p["bm"], p["bn"], p["sta"], p["stb"], p["prod"]) == (256, 128, 3, 2, 0)
    assert L.lib().ufnd_gemm_bf16_tile_info(30, None, None, None) == 0
