"""CPU: the video motion entries (csrc/motion.hip) and ultrafnd_git_amd/video.py refuse bad calls by name without touching a GPU."""
import numpy as np
import pytest
import torch

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def test_workspace_query_grows_with_the_frame_count():
    lib = _lib()
    one = lib.ufnd_motion_workspace_bytes(1, 2)
    assert one >= 2 * 65536
    assert lib.ufnd_motion_workspace_bytes(1, 8) > lib.ufnd_motion_workspace_bytes(1, 4) > one
    assert lib.ufnd_motion_workspace_bytes(4, 8) > lib.ufnd_motion_workspace_bytes(2, 8)
    assert lib.ufnd_motion_workspace_bytes(32, 30) >= 32 * 30 * 65536      # past 2^31 bytes at (32, 1200): a size_t
    assert lib.ufnd_motion_workspace_bytes(32, 1200) > 1 << 31
    for B, T in ((0, 4), (4, 0), (-1, 4), (1 << 13, 1 << 12)):
        assert lib.ufnd_motion_workspace_bytes(B, T) == 0, (B, T)


def test_gray_refusals():
    lib = _lib()
    err = lib.ufnd_last_error

    def call(frames=P, ws=P, B=2, T=3, H=40, W=48, strides=(17280, 5760, 1, 144, 3)):
        return lib.ufnd_motion_gray(frames, *strides, None, ws, B, T, H, W, None)

    assert call(frames=None) == 1 and b"null" in err()
    assert call(ws=None) == 1 and b"null" in err()
    assert call(B=0) == 1 and b"B=0" in err()
    assert call(T=0) == 1 and b"T=0" in err()
    assert call(B=1 << 13, T=1 << 12) == 1 and b"2^24" in err()
    assert call(H=0) == 1 and b"H=0" in err()
    assert call(W=-3) == 1 and b"W=-3" in err()
    assert call(strides=(17280, 5760, 1, -144, 3)) == 1 and b"negative stride" in err()
    assert call(ws=P + 8) == 1 and b"alignment" in err()


def test_pairs_and_finish_refusals():
    lib = _lib()
    err = lib.ufnd_last_error
    assert lib.ufnd_motion_pairs(None, None, 1, 4, 1, 3, None) == 1 and b"null" in err()
    assert lib.ufnd_motion_pairs(None, P, 0, 4, 1, 3, None) == 1 and b"B=0" in err()
    assert lib.ufnd_motion_pairs(None, P, 1, 0, 1, 3, None) == 1 and b"T=0" in err()
    for levels in (1, 2, 4, -1):
        assert lib.ufnd_motion_pairs(None, P, 1, 4, 1, levels, None) == 1 and f"levels={levels}".encode() in err()
    assert lib.ufnd_motion_pairs(None, P, 1, 4, 0, 0, None) == 1 and b"neither" in err()

    def chronos(ws=P, cut=P, flow=P, stats=P, feats=P, tamper=P, B=1, T=4, dim=128):
        return lib.ufnd_motion_chronos_finish(None, ws, cut, flow, stats, feats, tamper, B, T, dim, None)

    for kw in (dict(ws=None), dict(cut=None), dict(flow=None), dict(stats=None), dict(feats=None), dict(tamper=None)):
        assert chronos(**kw) == 1 and b"null" in err(), kw
    assert chronos(B=0) == 1 and b"B=0" in err()
    assert chronos(T=0) == 1 and b"T=0" in err()
    assert chronos(dim=0) == 1 and b"dim=0" in err()

    def flow(ws=P, feats=P, B=1, T=4, dim=256, levels=3):
        return lib.ufnd_motion_flow_finish(None, ws, None, feats, B, T, dim, levels, None)

    assert flow(ws=None) == 1 and b"null" in err()
    assert flow(feats=None) == 1 and b"null" in err()
    assert flow(B=-2) == 1 and b"B=-2" in err()
    assert flow(T=0) == 1 and b"T=0" in err()
    assert flow(dim=0) == 1 and b"dim=0" in err()
    assert flow(levels=2) == 1 and b"levels=2" in err()


def test_python_refusals_by_name():
    from ultrafnd_git_amd import video
    from ultrafnd_git_amd._lib import UltrafndHipError
    with pytest.raises(ValueError, match="n_pyramid_levels=2"):
        video.OpticalFlow3DCNN(n_pyramid_levels=2)
    flow, guard = video.OpticalFlow3DCNN(use_tvl1=True), video.ChronosGuard()
    assert flow.use_tvl1 is False and flow.dim == 256 and guard.feat_dim == 128
    with pytest.raises(TypeError, match="hash"):
        flow.extract("a title")
    with pytest.raises(TypeError, match="hash"):
        guard.extract_features("a title")
    clip = torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8)
    for call in (flow.extract_batch, guard.analyze_batch, guard.gray_frames, video.cache_visual):
        with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
            call(clip)
    with pytest.raises(UltrafndHipError, match="HIP device"):
        flow.extract_batch(np.zeros((1, 4, 8, 8, 3), np.uint8))


def test_layout_rule_and_channel_count():
    from ultrafnd_git_amd import video
    assert video.frame_layout((3, 40, 48)) == "CHW" and video.frame_layout((40, 48, 3)) == "HWC"
    assert video.frame_layout((3, 48, 3)) == "HWC"            # the reference's rule: shape[2] == 3 wins
    assert video.frame_layout((1, 40, 48)) == "CHW"
    meta = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device="meta")
    p = video._Plan(meta(2, 5, 3, 40, 48), None)
    assert (p.B, p.T, p.H, p.W) == (2, 5, 40, 48) and p.strides == (5 * 5760, 5760, 1920, 48, 1)
    p = video._Plan(meta(2, 5, 40, 48, 3), None)
    assert (p.H, p.W) == (40, 48) and p.strides == (5 * 5760, 5760, 1, 144, 3)
    p = video._Plan(meta(2, 5, 40, 48, 3).permute(0, 1, 4, 2, 3), None)      # CHW through a permuted view: no copy, the strides say it
    assert (p.H, p.W) == (40, 48) and p.strides == (5 * 5760, 5760, 1, 144, 3)
    p = video._Plan(meta(2, 5, 3, 48, 3), "CHW")                              # an explicit layout overrides the rule
    assert (p.H, p.W) == (48, 3)
    with pytest.raises(ValueError, match="1 channels"):
        video._Plan(meta(2, 5, 1, 40, 48), None)
    with pytest.raises(ValueError, match="4 channels"):
        video._Plan(meta(2, 5, 40, 48, 4), None)
    with pytest.raises(ValueError, match="expected"):
        video._Plan(meta(5, 40, 48, 3), None)
    with pytest.raises(ValueError, match="layout"):
        video._Plan(meta(2, 5, 40, 48, 3), "NHWC")


def test_estimate_av_lag_finds_a_shift():
    from ultrafnd_git_amd.video import ChronosGuard
    rng = np.random.default_rng(1)
    base = rng.standard_normal(400)
    for shift in (0, 3, 17):
        a, m = base[shift:shift + 300], base[:300]          # a[i] = m[i + shift]: the audio leads by `shift` samples
        assert ChronosGuard.estimate_av_lag(a, m, sr=100.0, max_lag_s=0.5) == pytest.approx(-shift / 100.0)
    assert ChronosGuard.estimate_av_lag(base[:3], base[:3]) == 0.0
