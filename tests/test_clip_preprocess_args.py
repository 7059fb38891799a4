"""CPU: the CLIP preprocessing entry (csrc/clip_preprocess.hip) and its Python layer (ultrafnd_git_amd/video.py, encoders.py) refuse bad
calls by name without touching a GPU; the header's limits are the ones _lib.py mirrors.  The entry needs no workspace: there is no
workspace query."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch
REPO = Path(__file__).resolve().parents[1]


def test_exported_constants_mirror_the_header():
    from ultrafnd_git_amd import _lib as L
    text = (REPO / "include" / "ultrafnd_hip.h").read_text()
    for name in ("MIN_SIZE", "MAX_SIZE", "MAX_TAPS", "MAX_SPAN", "MAX_TILE_ROWS", "INTER_BYTES", "INTER_BYTES_LARGE", "STAGE_BYTES", "MAX_EDGE"):
        assert int(re.search(rf"#define UFND_CLIP_PRE_{name} (\d+)", text).group(1)) == getattr(L, "CLIP_PRE_" + name), name
    assert re.search(r"#define UFND_CLIP_PRE_MAX_FRAMES \(1 << 24\)", text) and L.CLIP_PRE_MAX_FRAMES == 1 << 24
    assert L.CLIP_PRE_MIN_SIZE <= 224 <= L.CLIP_PRE_MAX_SIZE and L.CLIP_PRE_MAX_TAPS >= 41
    assert "int ufnd_clip_preprocess(const void* frames, long long stride_b" in text
    # the two workgroup sizes: lookup table + stage offsets + intermediate + stage
    assert 3072 + 128 + L.CLIP_PRE_INTER_BYTES + L.CLIP_PRE_STAGE_BYTES == 65536
    assert 3072 + 128 + L.CLIP_PRE_INTER_BYTES_LARGE + L.CLIP_PRE_STAGE_BYTES <= 160000
    assert 3 * (-(-L.CLIP_PRE_MAX_SPAN // 16) * 16 + 16) <= L.CLIP_PRE_STAGE_BYTES


def test_entry_refusals():
    from ultrafnd_git_amd import _lib as L
    lib = L.lib()
    err = lib.ufnd_last_error

    def call(frames=P, tab=P, vmap=P, pv=P, rgb=None, strides=(0, 0, 1, 3 * 1280, 3), B=2, T=3, H=720, W=1280, S=224, th=13, tv=13, x_lo=275, x_span=730,
             tile=15, rows=58):
        return lib.ufnd_clip_preprocess(frames, *strides, None, tab, vmap, pv, rgb, B, T, H, W, S, th, tv, x_lo, x_span, tile, rows, None)

    for key in ("frames", "tab", "vmap"):
        assert call(**{key: None}) == 1 and b"null" in err(), key
    assert call(pv=None) == 1 and b"no output" in err()
    for kw, msg in ((dict(B=0), b"B=0"), (dict(T=0), b"T=0"), (dict(B=-1), b"B=-1"), (dict(B=1 << 13, T=(1 << 11) + 1), b"T=2049"),
                    (dict(H=0), b"H=0"), (dict(W=0), b"W=0"), (dict(H=L.CLIP_PRE_MAX_EDGE + 1), b"H=65537"), (dict(W=-5), b"W=-5"),
                    (dict(S=L.CLIP_PRE_MIN_SIZE - 1), b"image_size=15"), (dict(S=L.CLIP_PRE_MAX_SIZE + 1), b"image_size=449"), (dict(S=0), b"image_size=0"),
                    (dict(th=0), b"taps_h=0"), (dict(th=L.CLIP_PRE_MAX_TAPS + 1), b"taps_h=65"), (dict(tv=L.CLIP_PRE_MAX_TAPS + 1), b"taps_v=65"),
                    (dict(tv=-1), b"taps_v=-1"), (dict(x_lo=-1), b"x_lo=-1"), (dict(x_span=0), b"x_span=0"), (dict(x_lo=600, x_span=730), b"x_span=730"),
                    (dict(W=8000, x_lo=0, x_span=L.CLIP_PRE_MAX_SPAN + 1), b"x_span=7001"), (dict(tile=0), b"tile_rows=0"),
                    (dict(tile=L.CLIP_PRE_MAX_TILE_ROWS + 1), b"tile_rows=17"), (dict(rows=0), b"lds_rows=0"), (dict(rows=721), b"lds_rows=721"),
                    (dict(rows=L.CLIP_PRE_INTER_BYTES_LARGE // 672 + 1), b"lds_rows=202"), (dict(B=1 << 12, T=1 << 12, tile=1), b"workgroups=3758096384"),
                    (dict(strides=(0, 0, 1, -3840, 3)), b"stride"), (dict(strides=(-1, 0, 1, 3840, 3)), b"stride"), (dict(tab=P + 2), b"alignment"),
                    (dict(vmap=P + 1), b"alignment"), (dict(pv=P + 3), b"alignment")):
        assert call(**kw) == 1 and msg in err(), (kw, err())
    assert call(pv=None, rgb=None) == 1


def test_python_refusals_by_name():
    from ultrafnd_git_amd import video
    from ultrafnd_git_amd._lib import UltrafndHipError
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    u8 = torch.zeros(2, 3, 40, 50, 3, dtype=torch.uint8)
    with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
        video.clip_preprocess(u8)
    with pytest.raises(UltrafndHipError, match="HIP device"):
        video.clip_preprocess(np.zeros((2, 3, 40, 50, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8 only"):
        video.clip_preprocess(u8.float())
    with pytest.raises(ValueError, match="uint8 only"):
        video.clip_preprocess(u8.to(torch.int16))
    with pytest.raises(ValueError, match="4 channels"):
        video.clip_preprocess(torch.zeros(2, 3, 40, 50, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 channels"):
        video.clip_preprocess(torch.zeros(2, 3, 1, 40, 50, dtype=torch.uint8), layout="CHW")
    with pytest.raises(ValueError, match="expected"):
        video.clip_preprocess(torch.zeros(40, 50, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="want='pixels'"):
        video.clip_preprocess(u8, want=("pixels",))
    with pytest.raises(ValueError, match="want is empty"):
        video.clip_preprocess(u8, want=())
    with pytest.raises(ValueError, match="image_size=8"):
        video.clip_preprocess(u8, image_size=8)
    with pytest.raises(ValueError, match="image_size=449"):
        video.clip_preprocess(u8, image_size=449)
    with pytest.raises(ValueError, match="std"):
        video.clip_preprocess(u8, std=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="mean"):
        video.clip_preprocess(u8, mean=(0.5, 0.5))
    with pytest.raises(ValueError, match="lengths holds 3"):
        video.clip_preprocess(u8, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match="taps"):      # 4000 -> 224: 2 ceil(2 * 17.86) + 1 = 73 taps
        video.clip_resize_tables(4000, 4000)
    # (a span past the limit needs a scale above 15.49 at image_size 448, a hair below where the tap count refuses: the entry's own refusal is
    # the one tested, in test_entry_refusals)
    with pytest.raises(ValueError, match="H=0"):
        video.clip_resize_tables(0, 10)
    assert video.clip_resize_tables(2160, 3840)["v"]["k"].shape[1] <= 41 and video.clip_resize_tables(3840, 2160)["lds_rows"] * 672 <= 135168
    sig = inspect.signature(video.clip_preprocess).parameters
    assert list(sig) == ["frames", "lengths", "layout", "image_size", "mean", "std", "want", "out"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, None, 224, video.CLIP_MEAN, video.CLIP_STD, ("pixel_values",), None]
    assert list(inspect.signature(video.clip_resize_tables).parameters) == ["H", "W", "image_size"]
    assert list(inspect.signature(ClipVisualEncoder.encode_frames).parameters) == ["self", "frames_u8", "lengths", "layout"]
    with pytest.raises(UltrafndHipError, match="HIP device only"):
        ClipVisualEncoder(layers=1).encode_frames(u8)
