"""CPU: the image-forgery entries (csrc/forgery.hip) and their classes in ultrafnd_git_amd/video.py refuse bad calls by name without
touching a GPU."""
import numpy as np
import pytest
import torch

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch
Q = bytes([16]) * 128


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def test_workspace_query():
    lib = _lib()
    one = lib.ufnd_forgery_workspace_bytes(1)
    assert one >= 3 * 196608 + 65536 + 2 * 16384
    assert lib.ufnd_forgery_workspace_bytes(32) >= 32 * one - 32 * 4096 and lib.ufnd_forgery_workspace_bytes(4) > lib.ufnd_forgery_workspace_bytes(2)
    assert lib.ufnd_forgery_workspace_bytes(1 << 16) > 1 << 31      # a size_t
    for B in (0, -1, (1 << 16) + 1):
        assert lib.ufnd_forgery_workspace_bytes(B) == 0, B


def test_entry_refusals():
    lib = _lib()
    err = lib.ufnd_last_error

    def resize(frames=P, ws=P, B=2, T=3, H=40, W=48, strides=(17280, 5760, 1, 144, 3)):
        return lib.ufnd_forgery_resize(frames, *strides, None, ws, B, T, H, W, None)

    assert resize(frames=None) == 1 and b"null" in err()
    assert resize(ws=None) == 1 and b"null" in err()
    assert resize(B=0) == 1 and b"B=0" in err()
    assert resize(B=(1 << 16) + 1) == 1 and b"65536" in err()
    assert resize(T=0) == 1 and b"T=0" in err()
    assert resize(H=0) == 1 and b"H=0" in err()
    assert resize(W=-3) == 1 and b"W=-3" in err()
    assert resize(strides=(17280, 5760, 1, -144, 3)) == 1 and b"negative stride" in err()
    assert resize(ws=P + 8) == 1 and b"alignment" in err()

    def trip(ws=P, q=Q, B=1, T=1, mode=1, slot=0):
        return lib.ufnd_forgery_roundtrip(None, ws, q, B, T, mode, slot, None)

    assert trip(ws=None) == 1 and b"null" in err()
    assert trip(q=None) == 1 and b"tables" in err()
    assert trip(q=bytes([16]) * 100 + bytes([0]) + bytes([16]) * 27) == 1 and b"quantiser 100" in err()
    assert trip(B=0) == 1 and b"B=0" in err()
    assert trip(mode=2) == 1 and b"jpeg_mode=2" in err()
    assert trip(slot=2) == 1 and b"slot=2" in err()
    assert trip(ws=P + 4) == 1 and b"alignment" in err()

    def maps(ws=P, scale=1.0, ela=None, gray=None, B=1, T=1, slot=0, lbp=1, grad=0):
        return lib.ufnd_forgery_maps(None, ws, scale, ela, gray, B, T, slot, lbp, grad, None)

    assert maps(ws=None) == 1 and b"null" in err()
    assert maps(T=0) == 1 and b"T=0" in err()
    assert maps(slot=-1) == 1 and b"slot=-1" in err()
    assert maps(scale=float("nan")) == 1 and b"finite" in err()
    assert maps(scale=float("inf")) == 1 and b"finite" in err()
    assert maps(slot=1, grad=1) == 1 and b"want_grad" in err()
    assert maps(ela=P + 2) == 1 and b"alignment" in err()

    def finish(ws=P, stats=P, lbp=P, feats=P, grad=P, score=P, B=1, T=1, dim=256, slot=0):
        return lib.ufnd_forgery_finish(None, ws, stats, lbp, feats, grad, score, B, T, dim, slot, None)

    assert finish(ws=None) == 1 and b"null" in err()
    assert finish(stats=None, lbp=None, feats=None, grad=None, score=None) == 1 and b"null" in err()
    assert finish(B=-2) == 1 and b"B=-2" in err()
    assert finish(dim=0) == 1 and b"dim=0" in err()
    assert finish(slot=3) == 1 and b"score_slot=3" in err()


def test_python_refusals_by_name():
    from ultrafnd_git_amd import video
    from ultrafnd_git_amd._lib import UltrafndHipError
    for q in (0, 101, -5):
        with pytest.raises(ValueError, match=f"ela_quality={q}"):
            video.DeepForgeryDetector(ela_quality=q)
    with pytest.raises(ValueError, match="jpeg="):
        video.DeepForgeryDetector(jpeg="turbo")
    with pytest.raises(ValueError, match="jpeg="):
        video.FaceWarpAnalyzer(jpeg="cv2")
    with pytest.raises(ValueError, match="dim=0"):
        video.DeepForgeryDetector(dim=0)
    with pytest.raises(ValueError, match="ela_scale"):
        video.DeepForgeryDetector(ela_scale=float("nan"))
    det, warp = video.DeepForgeryDetector(lbp_radius=2, lbp_points=16), video.FaceWarpAnalyzer()
    assert (det.dim, det.ela_quality, det.ela_scale, det.lbp_radius, det.lbp_points, det.jpeg) == (256, 85, 1.0, 2, 16, "libjpeg")
    with pytest.raises(TypeError, match="hash"):
        det.ela_lbp("a title")
    with pytest.raises(TypeError, match="hash"):
        warp.score("a title")
    clip = torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8)
    for call in (det.ela_lbp_batch, det.ela_map_batch, warp.score_batch, video.forgery_features):
        with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
            call(clip)
    with pytest.raises(UltrafndHipError, match="HIP device"):
        det.ela_lbp_batch(np.zeros((1, 4, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="ela_quality=0"):
        video.forgery_features(clip, ela_quality=0)


def test_quantisation_tables_follow_the_quality_rule():
    from ultrafnd_git_amd import video
    assert video.jpeg_qtables(50) == bytes(video.JPEG_K1 + video.JPEG_K2)
    assert set(video.jpeg_qtables(100)) == {1} and set(video.jpeg_qtables(1)) == {255}
    q85 = video.jpeg_qtables(85)
    assert len(q85) == 128 and q85[0] == 5 and q85[64] == 5 and q85[127] == 30
