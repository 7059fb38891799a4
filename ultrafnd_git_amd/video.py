"""Batched video motion forensics on the GPU: OpticalFlow3DCNN (src/core_blocks/visual_blocks.py:129-258) and ChronosGuard
(src/models/chronos_guard.py) of the reference, on the branches the reference itself takes on a host without OpenCV: nearest-neighbour
resize to 256 x 256, a float64 luma truncated to uint8, 32-bin frame histograms, |frame difference| as the flow, a 1-2-4 temporal
pyramid of per-pixel means with an 8-bin orientation histogram (csrc/motion.hip).  TV-L1 and Farneback flow are not built.

Frames: (B, T, H, W, 3) or (B, T, 3, H, W) on a HIP device, read through their strides (any view, no copy).  A frame is CHW by the
reference's rule -- shape[0] in (1, 3) and shape[2] != 3 -- unless layout= says otherwise; exactly 3 channels.  uint8 is the native
format; float frames are converted on the device by the reference's per-frame rule (a frame whose max is <= 1 + 1e-6 is scaled by 255;
then clip to 0..255 and truncate).  lengths: (B,) int32 on the device, clip b uses frames 0 .. lengths[b] - 1 and its results are the
bits of that clip alone; per-pair outputs are zero past a clip's last pair.

Degenerate clips give exactly what the reference gives, NaN included:
  fewer than 2 frames       zero vectors, score 0
  OpticalFlow3DCNN, 2-4 frames   the pyramid's finest level has four parts of max(1, pairs // 4) pairs; with fewer than 4 pairs one of
                            them is empty, its mean is NaN and normalisation spreads it: the whole vector is NaN (5 frames are finite)
  ChronosGuard.features     with more than 3 pairs the seventh statistic is np.corrcoef of the two per-pair series; a series without
                            variance (a static clip) makes it 0 / 0 = NaN and so the vector.  tamper_score does not use it and stays finite.
There is no CPU fallback: CPU tensors or a missing library raise.

Image-forgery evidence (csrc/forgery.hip): DeepForgeryDetector (:265-351) and FaceWarpAnalyzer (:358-406) of the same file.  Each clip
contributes one frame, index len // 2, resized to 256 x 256; a (B, H, W, 3) / (B, 3, H, W) image batch is a batch of one-frame clips.
The error level (ELA) map is |rgb - rec| with rec the frame after a JPEG round trip at `ela_quality`.  The reference makes that trip
through OpenCV; here it is baseline libjpeg's integer arithmetic on the device (4:2:0, standard tables, the islow DCTs, fancy
upsampling), equal to what libjpeg decodes in every byte -- jpeg="libjpeg".  jpeg="none" is the reference on a host without OpenCV:
rec = rgb, the map is zero and the vector a constant.  The LBP histogram is the reference's branch without scikit-image, the
gradient its forward differences.  A clip of length 0 gives a zero vector and score 0.0.

CLIP image preprocessing (csrc/clip_preprocess.hip): clip_preprocess() turns decoded uint8 frames into the (B, T, 3, 224, 224) float32
tensor ClipVisualEncoder takes, as the checkpoint's CLIPImageProcessor does on its Pillow backend (shortest-edge bicubic resize, centre
crop, rescale, normalise), equal to Pillow and the processor in every byte and float32 bit; clip_resize_tables() builds its
fixed-point coefficient tables on the host.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

SIDE = 256             # the reference's working size
POOLED = 77            # 7 pyramid chunks x (mean, std, max, 8 orientation counts)


def _as_clips(frames, device=None) -> torch.Tensor:
    """Frames of any rank -> the same frames as a device tensor; the callers check the rank (MotionStages: 5-D clips; ForgeryStages: 5-D
    clips or a 4-D image batch).  Host arrays and lists are moved to `device` (the single-input methods take what the reference's
    take); a CPU tensor is refused like everywhere in the package; a str raises."""
    if isinstance(frames, str):
        raise TypeError("a str input is the reference's salted-hash() text proxy, which is not reproduced: pass frames")
    if not isinstance(frames, torch.Tensor):
        if device is None:
            raise L.UltrafndHipError("frames must be a tensor on a HIP device (no CPU fallback)")
        frames = torch.from_numpy(np.ascontiguousarray(np.asarray(frames))).to(device)
    L.require_hip(frames)
    return frames


def frame_layout(frame_shape) -> str:
    """The reference's rule for one frame (_as_numpy_frame): CHW if shape[0] in (1, 3) and shape[2] != 3, else HWC."""
    return "CHW" if frame_shape[0] in (1, 3) and frame_shape[2] != 3 else "HWC"


def frames_to_uint8(frames: torch.Tensor) -> torch.Tensor:
    """The reference's per-frame conversion of non-uint8 frames, with torch ops on the device and no host synchronisation: a frame whose
    max is <= 1 + 1e-6 is scaled by 255; then clip to 0..255 and truncate.  uint8 frames pass through untouched."""
    if frames.dtype == torch.uint8:
        return frames
    if not frames.dtype.is_floating_point:
        frames = frames.float()
    peak = frames.amax(dim=(-3, -2, -1), keepdim=True)
    scale = torch.where(peak <= 1.0 + 1e-6, 255.0, 1.0).to(frames.dtype)
    return (frames * scale).clamp_(0, 255).to(torch.uint8)


class _Plan:
    """The strides of one call: (B, T, H, W) and element strides (b, t, c, y, x) of a 5-D uint8 tensor."""

    def __init__(self, frames: torch.Tensor, layout: Optional[str]):
        if frames.dim() != 5:
            raise ValueError(f"frames {tuple(frames.shape)}: expected (B, T, H, W, 3) or (B, T, 3, H, W)")
        lay = (layout or frame_layout(tuple(frames.shape[2:]))).upper()
        if lay not in ("HWC", "CHW"):
            raise ValueError(f"layout={layout!r}: 'HWC' or 'CHW'")
        s = frames.stride()
        B, T = frames.shape[:2]
        if lay == "CHW":
            Cn, H, W = frames.shape[2:]
            sc, sh, sw = s[2], s[3], s[4]
        else:
            H, W, Cn = frames.shape[2:]
            sh, sw, sc = s[2], s[3], s[4]
        if Cn != 3:
            raise ValueError(f"frames {tuple(frames.shape)} read as {lay}: {Cn} channels, exactly 3 (RGB) are supported")
        if B < 1 or T < 1 or H < 1 or W < 1:
            raise ValueError(f"frames {tuple(frames.shape)}: empty")
        self.B, self.T, self.H, self.W = int(B), int(T), int(H), int(W)
        self.strides = tuple(int(x) for x in (s[0], s[1], sc, sh, sw))


def _lengths(lengths, B: int, dev) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    lens = lengths.to(dev, torch.int32).contiguous() if isinstance(lengths, torch.Tensor) else torch.tensor(list(lengths), dtype=torch.int32, device=dev)
    if lens.numel() != B:
        raise ValueError(f"lengths holds {lens.numel()} entries for {B} clips")
    return lens


class MotionStages:
    """The three stages over one batch, sharing one workspace: gray -> pairs (+ pyramid) -> the two finishes.  Both classes below
    run on it; motion_features() runs everything once for callers that want both."""

    def __init__(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None):
        frames = frames_to_uint8(frames)
        self.dev = L.require_hip(frames)
        self.frames = frames                      # (kept alive until the launches are enqueued)
        self.plan = p = _Plan(frames, layout)
        self.lens = _lengths(lengths, p.B, self.dev)
        nbytes = L.lib().ufnd_motion_workspace_bytes(p.B, p.T)
        if nbytes == 0:
            raise L.UltrafndHipError(f"motion: B={p.B} T={p.T} is refused (B T <= 2^24)")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self._stream = L.stream_ptr(self.dev)

    def gray(self) -> torch.Tensor:
        p = self.plan
        L.check(L.lib().ufnd_motion_gray(self.frames.data_ptr(), *p.strides, L.ptr(self.lens), self.workspace.data_ptr(), p.B, p.T, p.H, p.W,
                                         self._stream), "ufnd_motion_gray")
        return self.workspace[:p.B * p.T * SIDE * SIDE].view(p.B, p.T, SIDE, SIDE)

    def pairs(self, pair_sums: bool, levels: int) -> None:
        p = self.plan
        L.check(L.lib().ufnd_motion_pairs(L.ptr(self.lens), self.workspace.data_ptr(), p.B, p.T, int(pair_sums), levels, self._stream), "ufnd_motion_pairs")

    def chronos(self, feat_dim: int) -> Dict[str, torch.Tensor]:
        p, dev = self.plan, self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"features": torch.empty(p.B, feat_dim, **f32), "tamper_score": torch.empty(p.B, **f32), "cut_scores": torch.empty(p.B, p.T - 1, **f32),
               "flow_mags": torch.empty(p.B, p.T - 1, **f32), "stats": torch.empty(p.B, 7, **f32)}
        L.check(L.lib().ufnd_motion_chronos_finish(L.ptr(self.lens), self.workspace.data_ptr(), out["cut_scores"].data_ptr() if p.T > 1 else None,
                                                   out["flow_mags"].data_ptr() if p.T > 1 else None, out["stats"].data_ptr(), out["features"].data_ptr(),
                                                   out["tamper_score"].data_ptr(), p.B, p.T, feat_dim, self._stream), "ufnd_motion_chronos_finish")
        return out

    def flow(self, dim: int, levels: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
        p, dev = self.plan, self.dev
        pooled = torch.empty(p.B, POOLED, dtype=torch.float32, device=dev)
        feats = torch.empty(p.B, dim, dtype=torch.float32, device=dev)
        L.check(L.lib().ufnd_motion_flow_finish(L.ptr(self.lens), self.workspace.data_ptr(), pooled.data_ptr(), feats.data_ptr(), p.B, p.T, dim, levels,
                                                self._stream), "ufnd_motion_flow_finish")
        return feats, pooled


@torch.no_grad()
def motion_features(frames: torch.Tensor, lengths=None, feat_dim: int = 128, dim: int = 256, layout: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """ChronosGuard.analyze_batch and OpticalFlow3DCNN.extract_batch over one gray pass and one walk through time: the dict of
    analyze_batch plus `flow` (B, dim) and `pooled` (B, 77)."""
    st = MotionStages(frames, lengths, layout)
    st.gray()
    st.pairs(True, 3)
    out = st.chronos(feat_dim)
    out["flow"], out["pooled"] = st.flow(dim)
    return out


class OpticalFlow3DCNN:
    """OpticalFlow3DCNN of the reference with its frame-difference flow: per pyramid chunk the mean, std and max of the per-pixel mean
    |d| and the 8-bin histogram of the per-pixel mean angle (77 values), tiled to `dim` and L2-normalised.

    n_pyramid_levels: 3 only.  use_tvl1 is accepted for signature compatibility and has no effect: neither TV-L1 nor Farneback is built,
    the flow is always the reference's frame-difference branch."""

    def __init__(self, dim: int = 256, n_pyramid_levels: int = 3, use_tvl1: bool = True, device="cuda"):
        if int(n_pyramid_levels) != 3:
            raise ValueError(f"n_pyramid_levels={n_pyramid_levels}: only the reference's default of 3 levels (1-2-4 parts) is built")
        if int(dim) < 1:
            raise ValueError(f"dim={dim}: at least 1")
        self.dim, self.n_pyr, self.use_tvl1 = int(dim), 3, False
        self.device = torch.device(device)

    @torch.no_grad()
    def extract_batch(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None, return_pooled: bool = False):
        """(B, dim) fp32 on the frames' device; with return_pooled also the (B, 77) values before tiling and normalisation."""
        st = MotionStages(_as_clips(frames), lengths, layout)
        st.gray()
        st.pairs(False, 3)
        feats, pooled = st.flow(self.dim)
        return (feats, pooled) if return_pooled else feats

    def extract(self, frames) -> np.ndarray:
        """One clip (T, H, W, 3) or (T, 3, H, W): a device tensor, or a host array / list of frames -> np.ndarray[dim]."""
        clip = _as_clips(frames, self.device)
        if clip.dim() != 4:
            raise ValueError(f"frames {tuple(clip.shape)}: one clip is (T, H, W, 3) or (T, 3, H, W)")
        return self.extract_batch(clip[None])[0].cpu().numpy()


class ChronosGuard:
    """ChronosGuard of the reference: per pair of frames a cut score (L1 distance of the two 32-bin density histograms) and a flow
    magnitude (mean |d|), seven statistics of the two series tiled to feat_dim and L2-normalised, and the heuristic tamper score."""

    def __init__(self, feat_dim: int = 128, device="cuda"):
        if int(feat_dim) < 1:
            raise ValueError(f"feat_dim={feat_dim}: at least 1")
        self.feat_dim = int(feat_dim)
        self.device = torch.device(device)

    @torch.no_grad()
    def analyze_batch(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """features (B, feat_dim), tamper_score (B,), cut_scores and flow_mags (B, T - 1), stats (B, 7) = mean, std, max of the cut
        scores, mean, std, max of the flow magnitudes, their correlation: all fp32 on the frames' device."""
        st = MotionStages(_as_clips(frames), lengths, layout)
        st.gray()
        st.pairs(True, 0)
        return st.chronos(self.feat_dim)

    @torch.no_grad()
    def gray_frames(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None) -> torch.Tensor:
        """The intermediate luma planes (B, T, 256, 256) uint8 (planes past a clip's length are not written)."""
        return MotionStages(_as_clips(frames), lengths, layout).gray()

    def _one(self, frames) -> Dict[str, torch.Tensor]:
        clip = _as_clips(frames, self.device)
        if clip.dim() != 4:
            raise ValueError(f"frames {tuple(clip.shape)}: one clip is (T, H, W, 3) or (T, 3, H, W)")
        return self.analyze_batch(clip[None])

    def extract_features(self, frames) -> np.ndarray:
        return self._one(frames)["features"][0].cpu().numpy()

    def temporal_tamper_score(self, frames, audio=None) -> float:
        """The score in [0, 1] (fp32 on the device).  `audio` is accepted and unused, as in the reference."""
        return float(self._one(frames)["tamper_score"][0].cpu())

    @staticmethod
    def estimate_av_lag(audio_env, mouth_open, sr: float = 16000.0, fps: float = 25.0, max_lag_s: float = 0.5) -> float:
        """Host-side NumPy.  The lag (seconds) at the peak of the cross-correlation of the two standardised envelopes, searched within
        +-max_lag_s: both cut to the shorter length n, correlated through a zero-padded FFT of the first power of two >= 2n, lags
        ordered -(n-1) .. n-1.  Fewer than 4 samples: 0.0.  (`fps` is unused, as in the reference.)"""
        a, m = np.asarray(audio_env), np.asarray(mouth_open)
        n = min(len(a), len(m))
        if n < 4:
            return 0.0
        a, m = a[:n], m[:n]
        a = (a - np.mean(a)) / (np.std(a) + 1e-9)
        m = (m - np.mean(m)) / (np.std(m) + 1e-9)
        nfft = 1
        while nfft < 2 * n:
            nfft *= 2
        xc = np.fft.irfft(np.fft.rfft(a, nfft) * np.conj(np.fft.rfft(m, nfft)), nfft)
        lags = np.concatenate([xc[nfft - (n - 1):], xc[:n]])
        mid, half = lags.size // 2, int(max_lag_s * sr)
        lo, hi = max(0, mid - half), min(lags.size, mid + half + 1)
        return float((lo + int(np.argmax(lags[lo:hi])) - mid) / sr)

    @staticmethod
    def estimate_av_lag_batch(audio_env, mouth_open, len_a=None, len_m=None, sr: float = 16000.0, fps: float = 25.0, max_lag_s: float = 0.5,
                              want=("lag_seconds",)) -> dict:
        """estimate_av_lag of a batch of pairs on the device: temporal.av_lag (device tensors in, device tensors out)."""
        from .temporal import av_lag
        return av_lag(audio_env, mouth_open, len_a, len_m, sr, fps, max_lag_s, want)


# ISO/IEC 10918-1 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural (row-major) order
JPEG_K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
JPEG_K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
SCORE_QUALITY = 85     # FaceWarpAnalyzer scores with DeepForgeryDetector(dim=16)'s map: quality 85, scale 1, whatever the caller's detector uses


def jpeg_qtables(quality: int) -> bytes:
    """libjpeg's quality rule over the two Annex-K tables -> 128 quantisers, luma then chroma, natural order."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"ela_quality={quality}: 1 .. 100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return bytes(min(255, max(1, (base * scale + 50) // 100)) for base in JPEG_K1 + JPEG_K2)


def _jpeg_mode(jpeg: str) -> int:
    if jpeg not in ("libjpeg", "none"):
        raise ValueError(f"jpeg={jpeg!r}: 'libjpeg' (the round trip) or 'none' (the reference without OpenCV: rec = rgb)")
    return int(jpeg == "libjpeg")


class ForgeryStages:
    """The stages over one batch, sharing one workspace: resize -> roundtrip -> maps -> finish.  Two slots hold a round-tripped image
    and its map partials each: slot 0 feeds the vector, `score_slot` the score's ELA term."""

    def __init__(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None):
        frames = frames_to_uint8(frames)
        if frames.dim() == 4:                     # an image batch: clips of one frame
            frames = frames.unsqueeze(1)
        self.dev = L.require_hip(frames)
        self.frames = frames                      # (kept alive until the launches are enqueued)
        self.plan = p = _Plan(frames, layout)
        self.lens = _lengths(lengths, p.B, self.dev)
        nbytes = L.lib().ufnd_forgery_workspace_bytes(p.B)
        if nbytes == 0:
            raise L.UltrafndHipError(f"forgery: B={p.B} is refused (B <= 65536)")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self._stream = L.stream_ptr(self.dev)

    def _image(self, k: int) -> torch.Tensor:
        n = self.plan.B * SIDE * SIDE * 3
        return self.workspace[k * n:(k + 1) * n].view(self.plan.B, SIDE, SIDE, 3)

    def resize(self) -> torch.Tensor:
        """The middle frames at the working size: (B, 256, 256, 3) uint8, a view of the workspace."""
        p = self.plan
        L.check(L.lib().ufnd_forgery_resize(self.frames.data_ptr(), *p.strides, L.ptr(self.lens), self.workspace.data_ptr(), p.B, p.T, p.H, p.W,
                                            self._stream), "ufnd_forgery_resize")
        return self._image(0)

    def roundtrip(self, quality: int, jpeg_mode: int = 1, slot: int = 0) -> torch.Tensor:
        """rec[slot] (B, 256, 256, 3) uint8, a view of the workspace."""
        p = self.plan
        tables = jpeg_qtables(quality) if jpeg_mode else None
        L.check(L.lib().ufnd_forgery_roundtrip(L.ptr(self.lens), self.workspace.data_ptr(), tables, p.B, p.T, jpeg_mode, slot, self._stream),
                "ufnd_forgery_roundtrip")
        return self._image(1 + slot)

    def maps(self, scale: float, slot: int = 0, lbp: bool = True, grad: bool = False, ela_map: bool = False, ela_gray: bool = False) -> Dict[str, torch.Tensor]:
        p = self.plan
        new = torch.empty if self.lens is None else torch.zeros      # an empty clip's map is not written: zeros
        out = {}
        if ela_map:
            out["ela_map"] = new(p.B, SIDE, SIDE, 3, dtype=torch.uint8, device=self.dev)
        if ela_gray:
            out["ela_gray"] = new(p.B, SIDE, SIDE, dtype=torch.uint8, device=self.dev)
        L.check(L.lib().ufnd_forgery_maps(L.ptr(self.lens), self.workspace.data_ptr(), float(scale), L.ptr(out.get("ela_map")), L.ptr(out.get("ela_gray")), p.B, p.T,
                                          slot, int(lbp), int(grad), self._stream), "ufnd_forgery_maps")
        return out

    def finish(self, dim: Optional[int] = None, grad: bool = False, score_slot: int = 0) -> Dict[str, torch.Tensor]:
        """dim: stats (B, 4), lbp (B, 10), features (B, dim); grad: grad (B, 2), score (B,)."""
        p = self.plan
        f32 = dict(dtype=torch.float32, device=self.dev)
        out = {}
        if dim is not None:
            out.update(stats=torch.empty(p.B, 4, **f32), lbp=torch.empty(p.B, 10, **f32), features=torch.empty(p.B, int(dim), **f32))
        if grad:
            out.update(grad=torch.empty(p.B, 2, **f32), score=torch.empty(p.B, **f32))
        L.check(L.lib().ufnd_forgery_finish(L.ptr(self.lens), self.workspace.data_ptr(), L.ptr(out.get("stats")), L.ptr(out.get("lbp")), L.ptr(out.get("features")),
                                            L.ptr(out.get("grad")), L.ptr(out.get("score")), p.B, p.T, int(dim or 1), score_slot, self._stream),
                "ufnd_forgery_finish")
        return out


@torch.no_grad()
def forgery_features(frames: torch.Tensor, lengths=None, dim: int = 256, ela_quality: int = 85, ela_scale: float = 1.0, jpeg: str = "libjpeg",
                     layout: Optional[str] = None, ela_map: bool = False) -> Dict[str, torch.Tensor]:
    """DeepForgeryDetector.ela_lbp_batch and FaceWarpAnalyzer.score_batch over one resize and, when the detector's settings are the
    score's (quality 85, scale 1), one round trip and one map: features (B, dim), stats (B, 4), lbp (B, 10), grad (B, 2), score (B,);
    with ela_map also the detector's map (B, 256, 256, 3) uint8."""
    mode = _jpeg_mode(jpeg)
    jpeg_qtables(ela_quality)
    st = ForgeryStages(_as_clips(frames), lengths, layout)
    st.resize()
    st.roundtrip(ela_quality, mode, 0)
    out = st.maps(ela_scale, 0, lbp=True, grad=True, ela_map=ela_map)
    score_slot = 0
    if mode and (int(ela_quality) != SCORE_QUALITY or float(ela_scale) != 1.0):
        score_slot = 1
        st.roundtrip(SCORE_QUALITY, mode, 1)
        st.maps(1.0, 1, lbp=False, grad=False)
    out.update(st.finish(dim, grad=True, score_slot=score_slot))
    return out


def _one_image(x, device) -> torch.Tensor:
    """What the reference's single-input methods take -> a batch of one clip: an image (H, W, 3) / (3, H, W), a stack of frames
    (T, H, W, 3) / (T, 3, H, W), or a list of frames."""
    if isinstance(x, (list, tuple)) and x and isinstance(x[0], torch.Tensor):
        x = torch.stack(list(x))
    clip = _as_clips(x, device)
    if clip.dim() == 3:
        clip = clip[None]
    if clip.dim() != 4:
        raise ValueError(f"input {tuple(clip.shape)}: one image (H, W, 3) or one stack of frames (T, H, W, 3), channels first or last")
    return clip[None]


class DeepForgeryDetector:
    """DeepForgeryDetector of the reference: [mean, std, max, min] of the ELA map and the 10-bin histogram of its luma's 3 x 3
    greater-neighbour counts, tiled to `dim` and L2-normalised.  lbp_radius and lbp_points are accepted and unused, as in the
    reference's branch without scikit-image."""

    def __init__(self, dim: int = 256, ela_quality: int = 85, ela_scale: float = 1.0, lbp_radius: int = 1, lbp_points: int = 8, jpeg: str = "libjpeg",
                 device="cuda"):
        if int(dim) < 1:
            raise ValueError(f"dim={dim}: at least 1")
        jpeg_qtables(ela_quality)
        if not np.isfinite(float(ela_scale)):
            raise ValueError(f"ela_scale={ela_scale}: finite")
        self.dim, self.ela_quality, self.ela_scale = int(dim), int(ela_quality), float(ela_scale)
        self.lbp_radius, self.lbp_points = int(lbp_radius), int(lbp_points)
        self.jpeg, self._mode = jpeg, _jpeg_mode(jpeg)
        self.device = torch.device(device)

    def _stages(self, frames, lengths, layout, **maps) -> Tuple[ForgeryStages, Dict[str, torch.Tensor]]:
        st = ForgeryStages(_as_clips(frames), lengths, layout)
        st.resize()
        st.roundtrip(self.ela_quality, self._mode, 0)
        return st, st.maps(self.ela_scale, 0, lbp=True, grad=False, **maps)

    @torch.no_grad()
    def ela_lbp_batch(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None, return_parts: bool = False):
        """(B, dim) fp32 on the frames' device; with return_parts also stats (B, 4) and lbp (B, 10)."""
        st, _ = self._stages(frames, lengths, layout)
        out = st.finish(self.dim)
        return (out["features"], out["stats"], out["lbp"]) if return_parts else out["features"]

    @torch.no_grad()
    def ela_map_batch(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None) -> torch.Tensor:
        """The ELA map itself, (B, 256, 256, 3) uint8 (zeros for a clip of length 0)."""
        return self._stages(frames, lengths, layout, ela_map=True)[1]["ela_map"]

    def ela_lbp(self, image_or_frames) -> np.ndarray:
        """One image or one stack of frames (its middle frame): a device tensor, or a host array / list -> np.ndarray[dim]."""
        return self.ela_lbp_batch(_one_image(image_or_frames, self.device))[0].cpu().numpy()


class FaceWarpAnalyzer:
    """FaceWarpAnalyzer of the reference: clip(0.5 tanh(g_std / (g_mean + 1e-6)) + 0.5 mean(ELA) / 255, 0, 1) with g the forward-difference
    gradient magnitude of the resized frame's luma and the ELA map that of a quality-85 round trip (zero with jpeg="none")."""

    def __init__(self, jpeg: str = "libjpeg", device="cuda"):
        self.jpeg, self._mode = jpeg, _jpeg_mode(jpeg)
        self.device = torch.device(device)

    @torch.no_grad()
    def score_batch(self, frames: torch.Tensor, lengths=None, layout: Optional[str] = None, return_parts: bool = False):
        """(B,) fp32 on the frames' device; with return_parts also grad (B, 2) = [g_mean, g_std]."""
        st = ForgeryStages(_as_clips(frames), lengths, layout)
        st.resize()
        st.roundtrip(SCORE_QUALITY, self._mode, 0)
        st.maps(1.0, 0, lbp=False, grad=True)
        out = st.finish(None, grad=True)
        return (out["score"], out["grad"]) if return_parts else out["score"]

    def score(self, image_or_frames) -> float:
        return float(self.score_batch(_one_image(image_or_frames, self.device))[0].cpu())


@torch.no_grad()
def cache_visual(frames: torch.Tensor, lengths=None, visual_dim: int = 512, layout: Optional[str] = None) -> torch.Tensor:
    """The `visual` row of the reference's cache builder: l2n(concat(flow(dim=visual_dim), ela)[:visual_dim]) with l2n(x) = x / (||x|| +
    1e-9).  The flow vector already fills visual_dim, so the ELA part (DeepForgeryDetector(dim=visual_dim)) is cut off whole and is
    not computed: (B, visual_dim) fp32."""
    x = OpticalFlow3DCNN(dim=visual_dim).extract_batch(frames, lengths, layout)
    return x / (torch.linalg.vector_norm(x, dim=1, keepdim=True) + 1e-9)


# ------------------------------------------------------------------ CLIP image preprocessing (csrc/clip_preprocess.hip)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # the processor's image_mean / image_std (OPENAI_CLIP_MEAN / _STD)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
CLIP_RESCALE = 0.00392156862745098                    # its rescale_factor: 1 / 255 as a double
_COEF_BITS = 22                                       # fractional bits of Pillow's fixed-point coefficients
_clip_tables_cache: dict = {}
_clip_tables_dev_cache: dict = {}
_clip_map_dev_cache: dict = {}


def _bicubic_weight(t: float) -> float:
    """Pillow's bicubic kernel, a = -0.5."""
    a = -0.5
    t = -t if t < 0.0 else t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def _pass_tables(n_in: int, n_out: int, lo: int, n: int) -> Dict[str, np.ndarray]:
    """Outputs lo .. lo + n - 1 of one resampling pass n_in -> n_out: first, count (n,) and k (n, taps) int32, built in float64 by
    Pillow's rule (include/ultrafnd_hip.h states it).  A pass with n_in == n_out is skipped by Pillow: the identity table."""
    if n_in == n_out:
        return {"first": np.arange(lo, lo + n, dtype=np.int32), "count": np.ones(n, np.int32), "k": np.full((n, 1), 1 << _COEF_BITS, np.int32), "skipped": True}
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, inv = 2.0 * fs, 1.0 / fs
    first, count, rows = np.zeros(n, np.int32), np.zeros(n, np.int32), []
    for i in range(n):
        c = (lo + i + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = max(min(int(c + support + 0.5), n_in), xmin)
        w = [_bicubic_weight((x + xmin - c + 0.5) * inv) for x in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        rows.append([int(v * (1 << _COEF_BITS) + 0.5) if v >= 0 else int(v * (1 << _COEF_BITS) - 0.5) for v in w])      # (int() truncates)
        first[i], count[i] = xmin, xmax - xmin
    k = np.zeros((n, max(1, int(count.max()))), np.int32)
    for i, r in enumerate(rows):
        k[i, :len(r)] = r
    assert int(np.abs(k).max()) < 1 << 23, "a normalised bicubic weight stays below 2: the kernel multiplies in 24 bits"
    return {"first": first, "count": count, "k": k, "skipped": False}


def clip_resize_tables(H: int, W: int, image_size: int = 224) -> dict:
    """Host only: the tables of CLIPImageProcessor's resize (shortest edge -> image_size, Pillow's bicubic) and centre crop for H x W
    sources, for the crop's rows and columns alone.
      resized (h', w'), top, left     the resized size and the crop's offsets in it
      h, v                            per pass (horizontal: W -> w', vertical: H -> h'): first, count (S,) int32, k (S, taps) int32
                                      (22 fractional bits), skipped (the pass has in == out: the identity table)
      x_lo, x_span                    the source columns the crop's horizontal taps reach
      tile_rows, lds_rows             output rows of a workgroup and the most intermediate rows one tile reaches: the largest tile of
                                      at most L.CLIP_PRE_MAX_TILE_ROWS rows whose intermediate fits L.CLIP_PRE_INTER_BYTES if that is at
                                      least 8 rows, else the largest that fits L.CLIP_PRE_INTER_BYTES_LARGE
      table                           the device form: hfirst, hcount, vfirst, vcount, hk, vk in one int32 array
    Cached per (H, W, image_size)."""
    H, W, S = int(H), int(W), int(image_size)
    if H < 1 or W < 1 or H > L.CLIP_PRE_MAX_EDGE or W > L.CLIP_PRE_MAX_EDGE:
        raise ValueError(f"clip_resize_tables: H={H} W={W} (1 .. {L.CLIP_PRE_MAX_EDGE} each)")
    if not L.CLIP_PRE_MIN_SIZE <= S <= L.CLIP_PRE_MAX_SIZE:
        raise ValueError(f"clip_resize_tables: image_size={S} ({L.CLIP_PRE_MIN_SIZE} .. {L.CLIP_PRE_MAX_SIZE})")
    key = (H, W, S)
    if key in _clip_tables_cache:
        return _clip_tables_cache[key]
    short, long_ = (W, H) if W <= H else (H, W)
    new_long = int(S * long_ / short)
    h2, w2 = (new_long, S) if W <= H else (S, new_long)
    top, left = (h2 - S) // 2, (w2 - S) // 2
    for name, n_in, n_out in (("horizontal", W, w2), ("vertical", H, h2)):
        taps = 2 * int(np.ceil(2.0 * max(n_in / n_out, 1.0))) + 1
        if n_in != n_out and taps > L.CLIP_PRE_MAX_TAPS:
            raise ValueError(f"clip_resize_tables: {H}x{W} -> {S}: the {name} pass has {taps} taps (at most {L.CLIP_PRE_MAX_TAPS}: the source is too large)")
    h, v = _pass_tables(W, w2, left, S), _pass_tables(H, h2, top, S)
    x_lo = int(h["first"].min())
    x_span = int((h["first"] + h["count"]).max()) - x_lo
    if x_span > L.CLIP_PRE_MAX_SPAN:
        raise ValueError(f"clip_resize_tables: {H}x{W} -> {S}: a row's taps reach {x_span} source columns (at most {L.CLIP_PRE_MAX_SPAN})")
    pitch = (3 * S + 3) // 4 * 4
    end = v["first"] + v["count"]

    def reach(tr):      # the most intermediate rows a tile of tr output rows needs
        return max(int(end[min(y0 + tr, S) - 1] - v["first"][y0]) for y0 in range(0, S, tr))

    fits = lambda limit: next((tr for tr in range(L.CLIP_PRE_MAX_TILE_ROWS, 0, -1) if reach(tr) * pitch <= limit), 0)
    tile_rows = fits(L.CLIP_PRE_INTER_BYTES)
    if tile_rows < 8:
        tile_rows = fits(L.CLIP_PRE_INTER_BYTES_LARGE)
    if tile_rows < 1:
        raise ValueError(f"clip_resize_tables: {H}x{W} -> {S}: one output row reaches {reach(1)} intermediate rows of {pitch} bytes "
                         f"(at most {L.CLIP_PRE_INTER_BYTES_LARGE} bytes)")
    table = np.concatenate([h["first"], h["count"], v["first"], v["count"], h["k"].ravel(), v["k"].ravel()]).astype(np.int32)
    out = {"H": H, "W": W, "image_size": S, "resized": (h2, w2), "top": top, "left": left, "h": h, "v": v, "x_lo": x_lo, "x_span": x_span,
           "tile_rows": tile_rows, "lds_rows": reach(tile_rows), "table": table}
    _clip_tables_cache[key] = out
    return out


def clip_value_map(mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """(3, 256) float32: what the processor's rescale + normalise make of byte v in channel c -- r = fl32(double(v) / 255-as-a-double
    product), then (r - fl32(mean)) / fl32(std) in fp32."""
    mean, std = np.asarray(mean, np.float64).ravel(), np.asarray(std, np.float64).ravel()
    if mean.size != 3 or std.size != 3 or not (np.isfinite(mean).all() and np.isfinite(std).all()) or (std.astype(np.float32) == 0).any():
        raise ValueError(f"clip_value_map: mean={tuple(mean)} std={tuple(std)} (3 finite values each, std non-zero)")
    r = (np.arange(256, dtype=np.float64) * CLIP_RESCALE).astype(np.float32)
    return ((r[None, :] - mean.astype(np.float32)[:, None]) / std.astype(np.float32)[:, None]).astype(np.float32)


def _dev_key(dev: torch.device):
    return (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())


@torch.no_grad()
def clip_preprocess(frames: torch.Tensor, lengths=None, layout: Optional[str] = None, image_size: int = 224, mean=CLIP_MEAN, std=CLIP_STD,
                    want=("pixel_values",), out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """The checkpoint's CLIPImageProcessor (Pillow backend: shortest-edge bicubic resize, centre crop, rescale, normalise) on decoded
    uint8 frames, in one launch, bit for bit: {"pixel_values": (B, T, 3, S, S) fp32 -- what ClipVisualEncoder takes -- and / or
    "rgb": (B, T, S, S, 3) uint8, the cropped resized image}, as `want` names them.
    frames: (B, T, H, W, 3) or (B, T, 3, H, W) uint8 on a HIP device, read through their strides (frames[:, ::k] subsamples for free);
    a 4-D image batch is a batch of one-frame clips.  lengths: (B,) frames per clip, never read on the host: a frame at or past its
    clip's length holds the bits of the clip's last valid frame, a clip of length 0 the image of an all-zero frame, and source frames
    at or past a length are not read.  out: {"pixel_values": ..., "rgb": ...} contiguous tensors of those shapes to write in place."""
    if isinstance(frames, str) or not torch.is_tensor(frames):
        raise L.UltrafndHipError("frames must be a tensor on a HIP device (no CPU fallback)")
    if frames.dtype != torch.uint8:
        raise ValueError(f"frames: dtype {frames.dtype} (uint8 only: the processor treats float images by a different arithmetic)")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want:
        raise ValueError("want is empty: 'pixel_values' and / or 'rgb'")
    for wname in want:
        if wname not in ("pixel_values", "rgb"):
            raise ValueError(f"want={wname!r}: 'pixel_values' and / or 'rgb'")
    if frames.dim() == 4:
        frames = frames.unsqueeze(1)
    p = _Plan(frames, layout)
    tab = clip_resize_tables(p.H, p.W, image_size)
    vmap = clip_value_map(mean, std)
    if lengths is not None and (lengths.numel() if torch.is_tensor(lengths) else len(lengths)) != p.B:
        raise ValueError(f"lengths holds {lengths.numel() if torch.is_tensor(lengths) else len(lengths)} entries for {p.B} clips")
    dev = L.require_hip(frames)
    S = tab["image_size"]
    lens = _lengths(lengths, p.B, dev)
    shapes = {"pixel_values": ((p.B, p.T, 3, S, S), torch.float32), "rgb": ((p.B, p.T, S, S, 3), torch.uint8)}
    res = {}
    for wname in want:
        shape, dtype = shapes[wname]
        t = None if out is None else out.get(wname)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"out[{wname!r}]: expected a contiguous {dtype} tensor of shape {shape} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        res[wname] = t
    key = (p.H, p.W, S) + _dev_key(dev)
    if key not in _clip_tables_dev_cache:
        _clip_tables_dev_cache[key] = torch.from_numpy(tab["table"]).to(dev)
    mkey = (vmap.tobytes(),) + _dev_key(dev)
    if mkey not in _clip_map_dev_cache:
        _clip_map_dev_cache[mkey] = torch.from_numpy(vmap).to(dev)
    table, vm = _clip_tables_dev_cache[key], _clip_map_dev_cache[mkey]
    L.check(L.lib().ufnd_clip_preprocess(frames.data_ptr(), *p.strides, L.ptr(lens), table.data_ptr(), vm.data_ptr(), L.ptr(res.get("pixel_values")),
                                         L.ptr(res.get("rgb")), p.B, p.T, p.H, p.W, S, tab["h"]["k"].shape[1], tab["v"]["k"].shape[1], tab["x_lo"],
                                         tab["x_span"], tab["tile_rows"], tab["lds_rows"], L.stream_ptr(dev)), "ufnd_clip_preprocess")
    return res
