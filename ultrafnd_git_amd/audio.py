"""Frozen, forward-only audio encoder that produces the `audio` (B, 128) input of the fusion step, MI355X-native.

  Wav2Vec2AudioEncoder  replaces SpectralForensics._w2v2_features (src/core_blocks/audio_blocks.py:111-139): utterance
                        normalisation (Wav2Vec2FeatureExtractor do_normalize) -> Wav2Vec2Model (wav2vec2-base geometry)
                        .last_hidden_state -> mean over time -> Linear(768, 128); batched over clips instead of one record at a
                        time on the CPU.
  SpectralForensics     the reference's class name and extract(audio, sr), bound to the encoder above (branch="w2v2", the default)
                        to the STFT statistics (branch="stft") or to the librosa descriptors (branch="librosa").
  spectral_descriptors, spectral_basis
                        the reference's librosa branches (_librosa_spectral's 11 descriptors, VoiceCloneDetector's descriptor mix) as
                        batched device kernels (csrc/spectral_desc.hip); restated from librosa's documented algorithms, not verified
                        against librosa.  SpectralForensics(branch="librosa"), VoiceCloneDetector(branch="librosa"),
                        cache_audio(branch="librosa").
  mel_spectrogram, mel_filterbank, mel_frame_count
                        the librosa branch of MelSpectrogramGenerator.generate: the 64-band mel spectrogram in dB (Slaney filterbank,
                        ref = the clip's maximum, floor -80) on the same STFT tile (csrc/mel_db.hip); restated, not verified against
                        librosa.  MelSpectrogramGenerator(branch="librosa").
  stft_forensics, MelSpectrogramGenerator, VoiceCloneDetector, cache_audio, wave_energy
                        the branches the reference takes without a checkpoint and without librosa (second half of this file,
                        csrc/spectral.hip): torch.stft(n_fft=400, hop_length=160) magnitudes -> statistics, 64 bands; the energy proxy.
  resample, resampled_length, resample_taps
                        the reference's _ensure_mono_16k (:34-45: channel mean + librosa.resample on the host) as a batched device
                        stage (csrc/resample.hip): polyphase windowed-sinc interpolation to 16 kHz.  Opt-in: the classes and
                        cache_audio take other rates only when given a `resample` quality.

Weights keep HF's `Wav2Vec2Model` state_dict names (plus proj.weight / proj.bias), so real checkpoints load unchanged.

Layout: frames are rows, channel-last, in per-clip slabs.  After conv layer 0 clip b owns rows
b S1 .. b S1 + T1_b - 1 of a (B S1, 512) bf16 buffer, S1 a multiple of 64; each stride-2 layer halves the slab, so ONE
overlapping-row GEMM launch per conv layer covers all clips and the transformer runs on slabs of S = S1 / 64 rows.  A valid
output row reads valid input rows only; slab-tail rows are garbage until the positional conv's add kernel zeroes them.

Every clip is computed as if it were alone: its own normalisation, GroupNorm statistics, attention keys and mean.  A clip's
feature is bit-identical alone and inside any batch, and from run to run (no atomics; fixed reduction trees; a GEMM row's
arithmetic does not depend on the tile it lands in).  No CPU path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .encoders import ACT_GELU, _bf16, _EncoderBase

CONV_KERNELS = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDES = (5, 2, 2, 2, 2, 2, 2)
CONV_DIM = 512
POS_KERNEL, POS_GROUPS = 128, 16
MIN_SAMPLES = L.AUDIO_MIN_SAMPLES
STAGES = ("conv0", "conv", "pos", "layers")


def frame_counts(n: int) -> List[int]:
    """Frames after each of the seven conv layers for a clip of n samples: T_out = (T_in - k) // s + 1."""
    out, t = [], int(n)
    for k, s in zip(CONV_KERNELS, CONV_STRIDES):
        t = (t - k) // s + 1
        out.append(t)
    return out


def frame_count(n: int) -> int:
    """Wav2Vec2Model._get_feat_extract_output_lengths for the wav2vec2-base geometry."""
    return frame_counts(n)[-1]


def slab_rows(n_max: int) -> int:
    """S1: rows of a clip's slab after conv layer 0 -- the frames of the longest clip rounded up to a multiple of 64."""
    return (frame_counts(n_max)[0] + 63) // 64 * 64


def tap_major(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight (out, in, k) -> (out, k in): the weight of the overlapping-row GEMM (row r = k in contiguous elements from
    frame s r on, channel-last)."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def resolve_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """The positional conv's weight_norm(dim=2) parametrisation: w = g v / ||v||, the norm over dims (0, 1) per tap;
    g = original0 (1, 1, k), v = original1 (out, in / groups, k)."""
    return g * v / v.norm(p=2, dim=(0, 1), keepdim=True)


def pos_group_weights(w: torch.Tensor, bias: torch.Tensor):
    """Grouped conv weight (768, 48, 128) and bias (768) -> per-group tap-major GEMM weights (16, 64, 128 * 48) and biases
    (16, 64): group g's 48 output rows padded with zero rows to the GEMM's 64-column granule."""
    G, k = POS_GROUPS, w.shape[2]
    co, ci = w.shape[0] // G, w.shape[1]
    wg = torch.zeros(G, 64, k * ci, dtype=w.dtype, device=w.device)
    bg = torch.zeros(G, 64, dtype=bias.dtype, device=bias.device)
    wg[:, :co] = w.view(G, co, ci, k).permute(0, 1, 3, 2).reshape(G, co, k * ci)
    bg[:, :co] = bias.view(G, co)
    return wg.contiguous(), bg.contiguous()


class Wav2Vec2AudioEncoder(_EncoderBase):
    LAYER_PREFIX = "encoder.layers.{}."
    LAYER_NAMES = {"qkv_w": [f"attention.{n}.weight" for n in ("q_proj", "k_proj", "v_proj")],
                   "qkv_b": [f"attention.{n}.bias" for n in ("q_proj", "k_proj", "v_proj")],
                   "o_w": ["attention.out_proj.weight"], "o_b": ["attention.out_proj.bias"], "g1": ["layer_norm.weight"], "b1n": ["layer_norm.bias"],
                   "w1": ["feed_forward.intermediate_dense.weight"], "b1": ["feed_forward.intermediate_dense.bias"],
                   "w2": ["feed_forward.output_dense.weight"], "b2": ["feed_forward.output_dense.bias"],
                   "g2": ["final_layer_norm.weight"], "b2n": ["final_layer_norm.bias"]}

    def __init__(self, layers: int = 12, hidden: int = 768, heads: int = 12, intermediate: int = 3072, out_dim: int = 128,
                 conv_dim: Sequence[int] = (CONV_DIM,) * 7, conv_kernel: Sequence[int] = CONV_KERNELS, conv_stride: Sequence[int] = CONV_STRIDES,
                 conv_bias: bool = False, feat_extract_norm: str = "group", num_conv_pos_embeddings: int = POS_KERNEL,
                 num_conv_pos_embedding_groups: int = POS_GROUPS, do_stable_layer_norm: bool = False, hidden_act: str = "gelu",
                 eps: float = 1e-5):
        # the wav2vec2-base geometry only (transformers.Wav2Vec2Config() defaults); anything else is refused by name
        for name, got, want in (("hidden", hidden, 768), ("heads", heads, 12), ("conv_dim", tuple(conv_dim), (CONV_DIM,) * 7),
                                ("conv_kernel", tuple(conv_kernel), CONV_KERNELS), ("conv_stride", tuple(conv_stride), CONV_STRIDES),
                                ("conv_bias", bool(conv_bias), False), ("feat_extract_norm", feat_extract_norm, "group"),
                                ("num_conv_pos_embeddings", num_conv_pos_embeddings, POS_KERNEL),
                                ("num_conv_pos_embedding_groups", num_conv_pos_embedding_groups, POS_GROUPS),
                                ("do_stable_layer_norm", bool(do_stable_layer_norm), False), ("hidden_act", hidden_act, "gelu")):
            if got != want:
                raise ValueError(f"{name}={got!r}: Wav2Vec2AudioEncoder is built for the wav2vec2-base geometry ({name}={want!r})")
        if intermediate % 64 or out_dim % 32 or layers < 1:
            raise ValueError(f"intermediate={intermediate} (a multiple of 64), out_dim={out_dim} (a multiple of 32), layers={layers} (>= 1)")
        super().__init__(hidden, heads, fold_ln=False, residual_dtype="fp32")      # the plain (unfolded-LayerNorm) layer form
        self.layers, self.inter, self.out_dim, self.eps = layers, intermediate, out_dim, eps
        w, init = self._w, self._seeded_init()
        F, E = "feature_extractor.conv_layers.", "encoder."
        cin = 1
        for i, k in enumerate(CONV_KERNELS):
            w[F + f"{i}.conv.weight"] = init((CONV_DIM, cin, k), std=(2.0 / (k * cin)) ** 0.5)      # (HF: kaiming_normal_)
            cin = CONV_DIM
        w[F + "0.layer_norm.weight"], w[F + "0.layer_norm.bias"] = torch.ones(CONV_DIM), torch.zeros(CONV_DIM)      # GroupNorm(512, 512)
        w["feature_projection.layer_norm.weight"], w["feature_projection.layer_norm.bias"] = torch.ones(CONV_DIM), torch.zeros(CONV_DIM)
        w["feature_projection.projection.weight"] = init((hidden, CONV_DIM))
        w["feature_projection.projection.bias"] = torch.zeros(hidden)
        v = init((hidden, hidden // POS_GROUPS, POS_KERNEL), std=2.0 * (1.0 / (POS_KERNEL * hidden)) ** 0.5)
        w[E + "pos_conv_embed.conv.bias"] = torch.zeros(hidden)
        w[E + "pos_conv_embed.conv.parametrizations.weight.original0"] = v.norm(p=2, dim=(0, 1), keepdim=True)
        w[E + "pos_conv_embed.conv.parametrizations.weight.original1"] = v
        w[E + "layer_norm.weight"], w[E + "layer_norm.bias"] = torch.ones(hidden), torch.zeros(hidden)
        for i in range(layers):
            P = E + f"layers.{i}."
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                w[P + f"attention.{n}.weight"] = init((hidden, hidden))
                w[P + f"attention.{n}.bias"] = torch.zeros(hidden)
            w[P + "layer_norm.weight"], w[P + "layer_norm.bias"] = torch.ones(hidden), torch.zeros(hidden)
            w[P + "feed_forward.intermediate_dense.weight"] = init((intermediate, hidden))
            w[P + "feed_forward.intermediate_dense.bias"] = torch.zeros(intermediate)
            w[P + "feed_forward.output_dense.weight"] = init((hidden, intermediate))
            w[P + "feed_forward.output_dense.bias"] = torch.zeros(hidden)
            w[P + "final_layer_norm.weight"], w[P + "final_layer_norm.bias"] = torch.ones(hidden), torch.zeros(hidden)
        w["proj.weight"] = init((out_dim, hidden))
        w["proj.bias"] = torch.zeros(out_dim)

    # ---- operands
    def _pack(self):
        if self._packed is None:
            # (HF scales q by 1 / sqrt(64) before Q K^T; the attention kernel scales the scores: the same product)
            w, F, E = self._w, "feature_extractor.conv_layers.", "encoder."
            pos_w = resolve_weight_norm(w[E + "pos_conv_embed.conv.parametrizations.weight.original0"],
                                        w[E + "pos_conv_embed.conv.parametrizations.weight.original1"])
            wg, bg = pos_group_weights(pos_w, w[E + "pos_conv_embed.conv.bias"])
            self._packed = {"layers": self._pack_layers(),
                            "w0": w[F + "0.conv.weight"].reshape(CONV_DIM, CONV_KERNELS[0]).contiguous(),
                            "conv": [_bf16(tap_major(w[F + f"{i}.conv.weight"])) for i in range(1, 7)],
                            "wfp": _bf16(w["feature_projection.projection.weight"]),
                            "wpos": _bf16(wg), "bpos": bg}
        return self._packed

    def _workbufs(self, B: int, n_max: int, S1: int) -> dict:
        """The work buffers of one pass as views of ONE grow-only store per buffer (self._bufs[name], flat): clip lengths vary freely
        (a cache builder sees a new n_max with almost every group), so nothing is keyed by the shape -- device memory is that of the
        largest pass seen, whatever the number of distinct lengths.  Slab strides come from S1, never from a store's size, so a row's
        bits do not depend on what ran before.  Nothing relies on a buffer's initial content."""
        dev, H, S = self.device, self.hidden, S1 // 64
        M, Sp = B * S, S1 // 64 + POS_KERNEL
        bf, f32, i32 = torch.bfloat16, torch.float32, torch.int32
        nwc, nfc = -(-n_max // L.WAVE_CHUNK), -(-S1 // L.CONV0_CHUNK)
        shapes = {
            "frames": ((B,), i32), "mask": ((B, S), i32),
            "xn": ((B, n_max), f32), "ws_wave": ((3 * B * nwc,), f32),
            "ws_conv0": ((3 * B * CONV_DIM * nfc + 2 * B * CONV_DIM,), f32),
            # conv ping-pong (+ 8 rows: the last slab's tail rows read up to k - 2 rows past their slab)
            "ca": ((B * S1 + 8, CONV_DIM), bf), "cb": ((B * S1 // 2 + 8, CONV_DIM), bf),
            "cf": ((M, CONV_DIM), f32), "fb": ((M, CONV_DIM), bf),
            "x0b": ((M, H), bf), "x0f": ((M, H), f32),
            "packed": ((POS_GROUPS, B * Sp + POS_KERNEL, H // POS_GROUPS), bf),
            "pconv": ((POS_GROUPS, B * Sp, 64), f32),
            "xb": ((M, H), bf), "xf": ((M, H), f32), "y": ((M, H), f32),
            "x1b": ((M, H), bf), "x1f": ((M, H), f32),
            "qkv": ((M, 3 * H), bf), "ctx": ((M, H), bf), "h": ((M, self.inter), bf),
            "pooled": ((B, H), f32), "feat": ((B, self.out_dim), f32)}
        views = {}
        for name, (shape, dt) in shapes.items():
            n = 1
            for d in shape:
                n *= d
            store = self._bufs.get(name)
            if store is None or store.numel() < n or store.device != dev:
                self._bufs[name] = store = torch.empty(n, dtype=dt, device=dev)
            views[name] = store[:n].view(shape)
        return views

    def workspace_bytes(self) -> int:
        """Device bytes the work buffers hold: those of the largest pass so far."""
        return sum(t.numel() * t.element_size() for t in self._bufs.values())

    def _conv_rows(self, A, W, bias, M, lda, out_bf16=None, out_f32=None):
        N, K = W.shape
        L.check(L.lib().ufnd_conv1d_rows_bf16(A.data_ptr(), W.data_ptr(), L.ptr(bias), L.ptr(out_bf16), L.ptr(out_f32), M, N, K, lda, W.stride(0),
                                              out_bf16.stride(0) if out_bf16 is not None else 0, out_f32.stride(0) if out_f32 is not None else 0,
                                              ACT_GELU, L.stream_ptr(A.device)), "ufnd_conv1d_rows_bf16")

    @staticmethod
    def _lengths(waves: torch.Tensor, lengths) -> List[int]:
        if waves.dim() != 2:
            raise ValueError(f"waves: expected (B, n_max), got {tuple(waves.shape)}")
        B, n_max = waves.shape
        lens = [n_max] * B if lengths is None else [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lens) != B:
            raise ValueError(f"lengths: {len(lens)} entries for {B} clips")
        for n in lens:
            if n < MIN_SAMPLES or n > n_max:
                raise ValueError(f"clip length {n}: at least {MIN_SAMPLES} samples (one output frame) and at most n_max={n_max}")
        return lens

    def _run(self, waves: torch.Tensor, lengths=None, n_layers: Optional[int] = None, stage: str = "layers", conv0_f32: Optional[torch.Tensor] = None,
             pool: bool = True):
        """One pass over (B, n_max) zero-padded clips up to `stage`: (work buffers, lengths, S1)."""
        lens = self._lengths(waves, lengths)
        self._require_hip()
        dev = self.device
        waves = waves[:, :max(lens)]      # (padding past the longest clip is never read)
        B, n_max = waves.shape
        S1 = slab_rows(n_max)
        S, M, H, s = S1 // 64, B * (S1 // 64), self.hidden, L.stream_ptr(dev)
        p, b, w, lib = self._pack(), self._workbufs(B, n_max, S1), self._w, L.lib()
        x = L.f32c(waves.to(dev))
        ln = torch.tensor(lens, dtype=torch.int32).to(dev)
        F = "feature_extractor.conv_layers."
        L.check(lib.ufnd_w2v2_frames(ln.data_ptr(), b["frames"].data_ptr(), b["mask"].data_ptr(), B, S, s), "ufnd_w2v2_frames")
        L.check(lib.ufnd_wave_normalize(x.data_ptr(), ln.data_ptr(), b["xn"].data_ptr(), b["ws_wave"].data_ptr(), B, n_max, s), "ufnd_wave_normalize")
        L.check(lib.ufnd_w2v2_conv0(b["xn"].data_ptr(), ln.data_ptr(), p["w0"].data_ptr(), w[F + "0.layer_norm.weight"].data_ptr(),
                                    w[F + "0.layer_norm.bias"].data_ptr(), b["ca"].data_ptr(), L.ptr(conv0_f32), b["ws_conv0"].data_ptr(), B, n_max, S1,
                                    self.eps, s), "ufnd_w2v2_conv0")
        if stage == "conv0":
            return b, lens, S1
        src, dst, rows = b["ca"], b["cb"], S1
        for i, W in enumerate(p["conv"]):      # layers 1-6: each halves the slab; ONE launch covers all clips
            rows //= 2
            if i < 5:
                self._conv_rows(src, W, None, B * rows, 2 * CONV_DIM, out_bf16=dst)
            else:
                self._conv_rows(src, W, None, B * rows, 2 * CONV_DIM, out_f32=b["cf"])      # (fp32: the LayerNorm that follows)
            src, dst = dst, src
        if stage == "conv":
            return b, lens, S1
        self._ln(b["cf"], CONV_DIM, w["feature_projection.layer_norm.weight"], w["feature_projection.layer_norm.bias"], b["fb"], None, M, CONV_DIM, self.eps)
        self._gemm(b["fb"], p["wfp"], w["feature_projection.projection.bias"], out_bf16=b["x0b"], out_f32=b["x0f"])
        # x + GELU(pos_conv(x)): pack -> 16 overlapping-row GEMMs (one per group) -> add; then encoder.layer_norm
        L.check(lib.ufnd_w2v2_pos_pack(b["x0b"].data_ptr(), b["frames"].data_ptr(), b["packed"].data_ptr(), B, S, s), "ufnd_w2v2_pos_pack")
        for g in range(POS_GROUPS):
            self._conv_rows(b["packed"][g], p["wpos"][g], p["bpos"][g], B * (S + POS_KERNEL), H // POS_GROUPS, out_f32=b["pconv"][g])
        L.check(lib.ufnd_w2v2_pos_add(b["x0f"].data_ptr(), b["pconv"].data_ptr(), b["frames"].data_ptr(), b["y"].data_ptr(), B, S, s), "ufnd_w2v2_pos_add")
        self._ln(b["y"], H, w["encoder.layer_norm.weight"], w["encoder.layer_norm.bias"], b["xb"], b["xf"], M, H, self.eps)
        if stage == "pos":
            return b, lens, S1
        layers = p["layers"] if n_layers is None else p["layers"][:max(1, int(n_layers))]
        self._post_ln_layers(layers, b, self._two_launch(b, "ufnd_attention_bf16", operands=(b["mask"],), B=B, Lq=S), M)      # (padded slabs, a key mask)
        if pool:
            L.check(lib.ufnd_masked_meanpool(b["xf"].data_ptr(), b["mask"].data_ptr(), b["pooled"].data_ptr(), B, S, H, s), "ufnd_masked_meanpool")
            L.check(lib.ufnd_linear_f32(b["pooled"].data_ptr(), w["proj.weight"].data_ptr(), w["proj.bias"].data_ptr(), b["feat"].data_ptr(), B,
                                        self.out_dim, H, s), "ufnd_linear_f32")
        return b, lens, S1

    @torch.no_grad()
    def normalized(self, waves: torch.Tensor, lengths=None) -> List[torch.Tensor]:
        """Wav2Vec2FeatureExtractor(do_normalize) of every clip: a list of (n_b,) fp32 tensors (for the tests)."""
        b, lens, _ = self._run(waves, lengths, stage="conv0")
        return [b["xn"][i, :n].clone() for i, n in enumerate(lens)]

    @torch.no_grad()
    def pooled(self, waves: torch.Tensor, lengths=None) -> torch.Tensor:
        """The mean over each clip's valid frames before the projection, (B, 768) fp32 (a copy; for the tests)."""
        return self._run(waves, lengths)[0]["pooled"].clone()

    @torch.no_grad()
    def last_hidden_state(self, waves: torch.Tensor, lengths=None, n_layers: Optional[int] = None, stage: str = "layers") -> List[torch.Tensor]:
        """Per clip, its valid frames (T_b, C) fp32 at a checkpoint (copies):
          stage="conv0"   conv layer 0 + GroupNorm + GELU before the bf16 rounding            (T1_b, 512)
          stage="conv"    the conv stack's output, extract_features before its LayerNorm      (T_b, 512)
          stage="pos"     after the positional conv and encoder.layer_norm                    (T_b, 768)
          stage="layers"  Wav2Vec2Model.hidden_states[n_layers] (all layers by default)       (T_b, 768)"""
        if stage not in STAGES:
            raise ValueError(f"stage={stage!r}: one of {STAGES}")
        if stage == "conv0":
            lens = self._lengths(waves, lengths)
            S1 = slab_rows(max(lens))
            f = torch.zeros(len(lens) * S1, CONV_DIM, dtype=torch.float32, device=self.device)
            self._run(waves, lengths, stage=stage, conv0_f32=f)
            return [f[i * S1:i * S1 + frame_counts(n)[0]].clone() for i, n in enumerate(lens)]
        b, lens, S1 = self._run(waves, lengths, n_layers=n_layers, stage=stage, pool=False)
        S, src = S1 // 64, b["cf"] if stage == "conv" else b["xf"]
        return [src[i * S:i * S + frame_count(n)].clone() for i, n in enumerate(lens)]

    @torch.no_grad()
    def forward(self, waves: torch.Tensor, lengths=None) -> torch.Tensor:
        """waves (B, n_max) fp32, zero-padded; lengths (B,) sample counts (default: all n_max) -> (B, out_dim) fp32 features
        (a view of an internal buffer, valid until the next call)."""
        return self._run(waves, lengths)[0]["feat"]


# ---------------------------------------------------------------------------------------------------------------------------
# The STFT branches (csrc/spectral.hip): what the reference computes on a host without librosa and without a wav2vec2 checkpoint.
N_FFT, HOP, N_BINS, N_BANDS = 400, 160, 201, 64
STFT_MIN_SAMPLES = L.STFT_MIN_SAMPLES      # torch.stft's reflect padding of 200 needs 201 samples
STFT_OUTPUTS = ("features", "stats", "mel_like", "magnitude", "frames")
_basis_cache: dict = {}


def dft_basis() -> np.ndarray:
    """(402, 400) float32: row k < 201 = cos(2 pi k n / 400), row 201 + k = -sin(2 pi k n / 400); the angle is reduced exactly
    (k n mod 400) and evaluated in float64, then rounded once."""
    kn = (np.arange(N_BINS, dtype=np.int64)[:, None] * np.arange(N_FFT, dtype=np.int64)[None, :]) % N_FFT
    ang = 2.0 * np.pi * kn.astype(np.float64) / N_FFT
    return np.concatenate([np.cos(ang), -np.sin(ang)]).astype(np.float32)


def _basis(dev: torch.device) -> torch.Tensor:
    """The basis on `dev`: built on the host once, uploaded once per device."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _basis_cache:
        _basis_cache[key] = torch.from_numpy(dft_basis()).to(dev)
    return _basis_cache[key]


def stft_frame_count(n: int) -> int:
    """T_b of a clip of n samples: 1 + n // 160, and 0 below 201 samples (torch.stft refuses those)."""
    return 1 + int(n) // HOP if int(n) >= STFT_MIN_SAMPLES else 0


def _device_waves(waves, lengths):
    """(B, n_max) or (B, C, n_max) on a HIP device -> ((B, n_max) fp32 contiguous, (B,) int32 lengths or None); channels are averaged
    on the device as the reference's _ensure_mono_16k does on the host."""
    if isinstance(waves, str):
        raise TypeError("a str (text proxy) is not supported: the reference's proxies use Python's salted hash(), so their values are not "
                        "reproducible from run to run")
    if not torch.is_tensor(waves):
        raise L.UltrafndHipError("waves must be a tensor on a HIP device (no CPU fallback)")
    dev = L.require_hip(waves)
    if waves.dim() == 3:
        waves = waves.float().mean(dim=1)
    if waves.dim() != 2 or waves.shape[0] < 1 or waves.shape[1] < 1:
        raise ValueError(f"waves: expected (B, n_max) or (B, C, n_max), got {tuple(waves.shape)}")
    B = waves.shape[0]
    lens = None
    if lengths is not None:
        lens = lengths.to(dev, torch.int32).contiguous() if torch.is_tensor(lengths) else torch.tensor(list(lengths), dtype=torch.int32, device=dev)
        if lens.numel() != B:
            raise ValueError(f"lengths holds {lens.numel()} entries for {B} clips")
    return L.f32c(waves), lens


@torch.no_grad()
def stft_forensics(waves: torch.Tensor, lengths=None, dim: int = 128, want: Sequence[str] = ("features",)) -> dict:
    """torch.stft(n_fft=400, hop_length=160).abs() of every clip and what the reference derives from it, in one launch plus a finish:
      features (B, dim)           SpectralForensics._torch_stft_fallback: [mean, std, max, min] tiled to dim, L2-normalised
      stats (B, 4)                mean, population std, max, min of |S|
      mel_like (B, 64, T_max)     MelSpectrogramGenerator's 3-bin pooling, [band, time], zeros past a clip's frames
      magnitude (B, 201, T_max)   |S| itself, zeros past a clip's frames
      frames (B,) int32           T_b = 1 + len_b // 160 (0 for a clip under 201 samples, whose outputs are all zeros)
    waves: (B, n_max) fp32 on a HIP device, or (B, C, n_max), averaged to mono; lengths: (B,) samples per clip (a device tensor is not
    read on the host: nothing here synchronises).  features and stats never write the spectrogram."""
    want = tuple(want)
    for name in want:
        if name not in STFT_OUTPUTS:
            raise ValueError(f"want={name!r}: one of {STFT_OUTPUTS}")
    if not want:
        raise ValueError(f"want is empty: some of {STFT_OUTPUTS}")
    if int(dim) < 1:
        raise ValueError(f"dim={dim}: at least 1")
    x, lens = _device_waves(waves, lengths)
    dev, (B, n_max) = x.device, x.shape
    T_max = 1 + n_max // HOP
    f32 = dict(dtype=torch.float32, device=dev)
    out = {}
    if "features" in want:
        out["features"] = torch.empty(B, int(dim), **f32)
    if "stats" in want:
        out["stats"] = torch.empty(B, 4, **f32)
    if "mel_like" in want:
        out["mel_like"] = torch.empty(B, N_BANDS, T_max, **f32)
    if "magnitude" in want:
        out["magnitude"] = torch.empty(B, N_BINS, T_max, **f32)
    if out:
        ws = None
        if "features" in out or "stats" in out:
            nbytes = L.lib().ufnd_spectral_workspace_bytes(B, n_max)
            if nbytes == 0:
                raise L.UltrafndHipError(f"stft_forensics: B={B} n_max={n_max} is refused (B <= 65535, n_max <= 2^30)")
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        L.check(L.lib().ufnd_stft_forensics(x.data_ptr(), L.ptr(lens), _basis(dev).data_ptr(), L.ptr(ws), L.ptr(out.get("magnitude")),
                                            L.ptr(out.get("mel_like")), L.ptr(out.get("stats")), L.ptr(out.get("features")), B, n_max, int(dim),
                                            L.stream_ptr(dev)), "ufnd_stft_forensics")
    if "frames" in want:
        n = torch.full((B,), n_max, dtype=torch.int32, device=dev) if lens is None else lens.clamp(0, n_max)
        out["frames"] = torch.where(n >= STFT_MIN_SAMPLES, 1 + torch.div(n, HOP, rounding_mode="floor"), torch.zeros_like(n)).to(torch.int32)
    return out


@torch.no_grad()
def wave_energy(waves: torch.Tensor, lengths=None) -> dict:
    """energy (B,) = mean(x^2) and score (B,) = clip(e / (e + 1), 0, 1): VoiceCloneDetector's energy proxy, batched."""
    x, lens = _device_waves(waves, lengths)
    B, n_max = x.shape
    out = {"energy": torch.empty(B, dtype=torch.float32, device=x.device), "score": torch.empty(B, dtype=torch.float32, device=x.device)}
    L.check(L.lib().ufnd_wave_energy(x.data_ptr(), L.ptr(lens), out["energy"].data_ptr(), out["score"].data_ptr(), B, n_max, L.stream_ptr(x.device)),
            "ufnd_wave_energy")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The librosa branches (csrc/spectral_desc.hip): what the reference computes on a host WITH librosa and without a checkpoint.
# Restated from librosa's documented algorithms (0.10 defaults), not verified against librosa itself (include/ultrafnd_hip.h).
DESC_GEOMETRY = {400: 160, 2048: 512}      # n_fft: hop of the two STFTs of _librosa_spectral
N_DESCRIPTORS, N_CONTRAST_BANDS = 11, 7
DESC_OUTPUTS = ("features", "descriptors", "contrast", "flatness", "centroid", "rolloff", "flatness_y", "zcr", "clone_score", "magnitude",
                "magnitude_y")
_desc_basis_cache: dict = {}


def spectral_basis(n_fft: int) -> np.ndarray:
    """(2 (n_fft / 2 + 1), n_fft) float32, n_fft 400 or 2048: row k = w[n] cos(2 pi k n / n_fft), row n_fft / 2 + 1 + k =
    -w[n] sin(2 pi k n / n_fft) with the periodic Hann window w[n] = 0.5 - 0.5 cos(2 pi n / n_fft); the angle is reduced exactly
    (k n mod n_fft), everything is evaluated in float64 and the product is rounded once."""
    if n_fft not in DESC_GEOMETRY:
        raise ValueError(f"n_fft={n_fft!r}: spectral_basis is built for {tuple(DESC_GEOMETRY)} (other n_fft / hop are not built)")
    n = np.arange(n_fft, dtype=np.int64)
    kn = (np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None] * n[None, :]) % n_fft
    ang = 2.0 * np.pi * kn.astype(np.float64) / n_fft
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n.astype(np.float64) / n_fft)
    return np.concatenate([np.cos(ang) * win, -np.sin(ang) * win]).astype(np.float32)


def _desc_basis(dev: torch.device, n_fft: int) -> torch.Tensor:
    key = (n_fft, dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _desc_basis_cache:
        _desc_basis_cache[key] = torch.from_numpy(spectral_basis(n_fft)).to(dev)
    return _desc_basis_cache[key]


def desc_frame_counts(n: int):
    """(T_A, T_B) of a clip of n samples: 1 + n // 160 and 1 + n // 512 (zero padding: any n >= 1 has frames), (0, 0) for n = 0."""
    return (1 + int(n) // 160, 1 + int(n) // 512) if int(n) >= 1 else (0, 0)


@torch.no_grad()
def spectral_descriptors(waves: torch.Tensor, lengths=None, dim: int = 128, want: Sequence[str] = ("features",), pad_mode: str = "constant") -> dict:
    """SpectralForensics._librosa_spectral and VoiceCloneDetector's librosa score of every 16 kHz clip, batched:
      features (B, dim)             the 11 descriptors tiled to dim, L2-normalised
      descriptors (B, 11)           |S| mean, std, max, min; contrast mean, std; flatness mean, std; mean centroid, rolloff, zcr
      contrast (B, 7, T_A_max)      spectral_contrast(S, sr=16000)            } of librosa.stft(n_fft=400, hop_length=160),
      flatness (B, T_A_max)         spectral_flatness(S)                      } T_A = 1 + len // 160
      magnitude (B, 201, T_A_max)   S itself                                  }
      centroid, rolloff, flatness_y, zcr (B, T_B_max)     the y= forms: n_fft 2048, hop 512, T_B = 1 + len // 512
      magnitude_y (B, 1025, T_B_max)                      their magnitudes
      clone_score (B,)              clip(0.4 mean(flatness_y) + 0.3 mean(zcr) + 0.3 tanh(mean(centroid) / 3000), 0, 1)
    Per-frame outputs hold zeros from a clip's own frame count on; a clip of length 0 gives zeros everywhere.
    waves, lengths: as stft_forensics (a device `lengths` is not read on the host: nothing here synchronises).  Outputs that are not
    asked for are not stored, and what is asked for does not change any value's bits.  pad_mode: librosa >= 0.10's "constant" (zero
    padding) only."""
    if pad_mode != "constant":
        raise ValueError(f"pad_mode={pad_mode!r}: only 'constant' (zero padding, librosa >= 0.10's default) is built; 'reflect' is not")
    want = tuple(want)
    for name in want:
        if name not in DESC_OUTPUTS:
            raise ValueError(f"want={name!r}: one of {DESC_OUTPUTS}")
    if not want:
        raise ValueError(f"want is empty: some of {DESC_OUTPUTS}")
    if int(dim) < 1:
        raise ValueError(f"dim={dim}: at least 1")
    x, lens = _device_waves(waves, lengths)
    dev, (B, n_max) = x.device, x.shape
    TA, TB = 1 + n_max // 160, 1 + n_max // 512
    shapes = {"features": (B, int(dim)), "descriptors": (B, N_DESCRIPTORS), "contrast": (B, N_CONTRAST_BANDS, TA), "flatness": (B, TA),
              "centroid": (B, TB), "rolloff": (B, TB), "flatness_y": (B, TB), "zcr": (B, TB), "clone_score": (B,), "magnitude": (B, 201, TA),
              "magnitude_y": (B, 1025, TB)}
    out = {name: torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in DESC_OUTPUTS if name in want}
    nbytes = L.lib().ufnd_spectral_desc_workspace_bytes(B, n_max)
    if nbytes == 0:
        raise L.UltrafndHipError(f"spectral_descriptors: B={B} n_max={n_max} is refused (B <= 65535, n_max <= 2^30)")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    io = L.SpectralDescOut(**{name: t.data_ptr() for name, t in out.items()})
    L.check(L.lib().ufnd_spectral_descriptors(x.data_ptr(), L.ptr(lens), _desc_basis(dev, 400).data_ptr(), _desc_basis(dev, 2048).data_ptr(),
                                              ws.data_ptr(), io, B, n_max, int(dim), L.stream_ptr(dev)), "ufnd_spectral_descriptors")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The librosa branch of MelSpectrogramGenerator (csrc/mel_db.hip): power_to_db(melspectrogram(y, sr=16000, n_fft=400, hop_length=160,
# n_mels=64), ref=np.max).  Restated from librosa's documented algorithms (0.10 defaults), not verified against librosa itself
# (include/ultrafnd_hip.h); the filterbank alone is checked against an independent implementation (tests/test_mel_ref.py).
MEL_OUTPUTS = ("mel_db", "mel_power", "mel_max")
MEL_FMIN, MEL_FMAX = 0.0, 8000.0
_mel_fb_host: dict = {}
_mel_fb_cache: dict = {}


def _slaney_mel(f):
    """Hz -> mel on the Slaney scale (htk=False): 3 f / 200 below 1000 Hz, 15 + 27 ln(f / 1000) / ln 6.4 from 1000 Hz on."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)


def _slaney_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (np.maximum(m, 15.0) - 15.0)), 200.0 * m / 3.0)


def mel_points() -> np.ndarray:
    """m[0 .. 65] in Hz (float64): 66 points equally spaced in mel over [mel(0), mel(8000)]."""
    return _slaney_hz(np.linspace(float(_slaney_mel(MEL_FMIN)), float(_slaney_mel(MEL_FMAX)), N_BANDS + 2))


def mel_filterbank() -> dict:
    """librosa.filters.mel(sr=16000, n_fft=400, n_mels=64) (fmin 0, fmax 8000, htk=False, norm="slaney"), restated:
      weights (64, 201) float32   W[i, k] = max(0, min((40 k - m[i]) / (m[i+1] - m[i]), (m[i+2] - 40 k) / (m[i+2] - m[i+1])))
                                  2 / (m[i+2] - m[i]), evaluated in float64 and rounded once
      first, count (64,) int32    every row's support is contiguous: bins first .. first + count - 1
      packed (388,) float32       the nonzeros, row after row: what the device reads
    Built once; the same (read-only) arrays are returned on every call."""
    if not _mel_fb_host:
        m = mel_points()
        freq = np.linspace(0.0, 8000.0, N_BINS)      # 40 k Hz, exact
        diff = np.diff(m)
        slopes = m[None, :] - freq[:, None]      # (201, 66)
        down, up = -slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]
        w64 = np.maximum(0.0, np.minimum(down, up)) * (2.0 / (m[2:] - m[:-2]))
        w = np.ascontiguousarray(w64.T.astype(np.float32))
        first = np.array([np.flatnonzero(r)[0] for r in w], dtype=np.int32)
        count = np.array([np.count_nonzero(r) for r in w], dtype=np.int32)
        packed = np.concatenate([w[i, first[i]:first[i] + count[i]] for i in range(N_BANDS)])
        if len(packed) != L.MEL_NNZ or np.count_nonzero(packed) != L.MEL_NNZ:
            raise L.UltrafndHipError(f"mel_filterbank: {np.count_nonzero(packed)} nonzeros in contiguous supports, the kernel is built for {L.MEL_NNZ}")
        for a in (w, first, count, packed):
            a.setflags(write=False)
        _mel_fb_host.update(weights=w, first=first, count=count, packed=packed)
    return dict(_mel_fb_host)


def _mel_fb(dev: torch.device):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _mel_fb_cache:
        fb = mel_filterbank()
        _mel_fb_cache[key] = tuple(torch.from_numpy(fb[k].copy()).to(dev) for k in ("packed", "first", "count"))
    return _mel_fb_cache[key]


def mel_frame_count(n: int) -> int:
    """T of a clip of n samples: 1 + n // 160 (zero padding: any n >= 1 has frames), 0 for n = 0."""
    return 1 + int(n) // HOP if int(n) >= 1 else 0


@torch.no_grad()
def mel_spectrogram(waves: torch.Tensor, lengths=None, want: Sequence[str] = ("mel_db",)) -> dict:
    """MelSpectrogramGenerator.generate's librosa branch of every 16 kHz clip, batched (T = 1 + len // 160, T_max = 1 + n_max // 160):
      mel_db (B, 64, T_max)      power_to_db(melspectrogram(y, sr=16000, n_fft=400, hop_length=160, n_mels=64, power=2.0), ref=np.max):
                                 10 log10(max(1e-10, M)) - 10 log10(max(1e-10, max M)), floored at -80; the maximum is the clip's own
      mel_power (B, 64, T_max)   M = W S^2, S the magnitudes of spectral_descriptors (the same bits)
      mel_max (B,)               the clip's largest M
    Per-frame outputs hold zeros from a clip's own T on -- 0 is also a legitimate dB value (the clip's loudest entry), so cut a clip
    by mel_frame_count; a clip of length 0 gives zeros everywhere, an all-zero clip 0 dB on its frames.  waves, lengths: as
    spectral_descriptors (a device `lengths` is not read on the host: nothing here synchronises).  What is asked for changes no
    value's bits."""
    want = tuple(want)
    for name in want:
        if name not in MEL_OUTPUTS:
            raise ValueError(f"want={name!r}: one of {MEL_OUTPUTS}")
    if not want:
        raise ValueError(f"want is empty: some of {MEL_OUTPUTS}")
    x, lens = _device_waves(waves, lengths)
    dev, (B, n_max) = x.device, x.shape
    T_max = 1 + n_max // HOP
    shapes = {"mel_db": (B, N_BANDS, T_max), "mel_power": (B, N_BANDS, T_max), "mel_max": (B,)}
    out = {name: torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in MEL_OUTPUTS if name in want}
    nbytes = L.lib().ufnd_mel_workspace_bytes(B, n_max)
    if nbytes == 0:
        raise L.UltrafndHipError(f"mel_spectrogram: B={B} n_max={n_max} is refused (B <= 65535, n_max <= 2^30)")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    packed, first, count = _mel_fb(dev)
    L.check(L.lib().ufnd_mel_spectrogram(x.data_ptr(), L.ptr(lens), _desc_basis(dev, 400).data_ptr(), packed.data_ptr(), first.data_ptr(),
                                         count.data_ptr(), ws.data_ptr(), L.ptr(out.get("mel_db")), L.ptr(out.get("mel_power")),
                                         L.ptr(out.get("mel_max")), B, n_max, L.stream_ptr(dev)), "ufnd_mel_spectrogram")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Sample-rate conversion (csrc/resample.hip): the stage between a decoded waveform and the 16 kHz entries of this file.
RESAMPLE_QUALITIES = {      # name: (lowpass_filter_width, rolloff, kaiser beta or None for the Hann window)
    "kaiser_best": (64, 0.9475937167399596, 14.769656459379492),      # the set published as equivalent to resampy's kaiser_best
    "kaiser_fast": (16, 0.85, 8.555504641634386),
    "hann": (6, 0.99, None)}
RESAMPLE_MAX_TABLE_FLOATS = 1 << 22      # the device table of one (rate pair, quality): fewer strides are folded above this
_taps_cache: dict = {}
_taps_dev_cache: dict = {}


def _rate_ratio(orig_sr, new_sr):
    """(o, n): the reduced ratio orig_sr / new_sr; refuses by name what the resampler does not take."""
    for name, v in (("orig_sr", orig_sr), ("new_sr", new_sr)):
        ok = not isinstance(v, bool) and (isinstance(v, (int, np.integer)) or (isinstance(v, (float, np.floating)) and float(v).is_integer()))
        if not ok or int(v) <= 0:
            raise ValueError(f"{name}={v!r}: a sample rate is a positive integer (Hz)")
    g = int(np.gcd(int(orig_sr), int(new_sr)))
    o, n = int(orig_sr) // g, int(new_sr) // g
    if o > L.RESAMPLE_MAX_RATIO_TERM or n > L.RESAMPLE_MAX_RATIO_TERM:
        raise ValueError(f"orig_sr={int(orig_sr)} -> new_sr={int(new_sr)}: the reduced ratio {o}/{n} has a term above {L.RESAMPLE_MAX_RATIO_TERM} "
                         "(the limit that bounds the tap table)")
    return o, n


def _quality(quality):
    if not isinstance(quality, str) or quality not in RESAMPLE_QUALITIES:
        raise ValueError(f"quality={quality!r}: one of {tuple(RESAMPLE_QUALITIES)}")
    return RESAMPLE_QUALITIES[quality]


def resampled_length(n: int, orig_sr: int, new_sr: int = 16000) -> int:
    """Samples a clip of n samples has after resampling: ceil(new n / orig) on the reduced ratio, the device's formula."""
    o, m = _rate_ratio(orig_sr, new_sr)
    if int(n) < 0:
        raise ValueError(f"n={n}: a clip length is at least 0")
    return (m * int(n) + o - 1) // o


def _device_table(h: np.ndarray, first: np.ndarray, count: np.ndarray, o: int, n: int, K: int) -> dict:
    """The tables ufnd_resample reads (include/ultrafnd_hip.h): G strides folded into one super-stride, groups of 4 phases."""
    lds, qt_max = L.RESAMPLE_LDS_FLOATS, L.RESAMPLE_OUT_TILE
    G = max(1, 64 // n)
    G -= 1 - G % 2      # odd: o' = G o stays odd when o is, and the lanes' LDS reads spread over all banks
    while G > 1 and (G * n * (K + (G - 1) * o) > RESAMPLE_MAX_TABLE_FLOATS or (qt_max - 1) * G * o + 1024 > lds):
        G -= 2
    np_, op = G * n, G * o
    sfirst = np.concatenate([first + g * o for g in range(G)])      # phase g n + p of the super-stride: phase p shifted by g o taps
    scount = np.tile(count, G)
    ngroups = -(-np_ // 4)
    groups = np.zeros((ngroups, 3), dtype=np.int32)
    rows = 0
    for g in range(ngroups):
        ph = slice(4 * g, min(4 * g + 4, np_))
        lo = int(sfirst[ph].min()) // 8 * 8
        hi = -(-int((sfirst[ph] + scount[ph]).max()) // 8) * 8
        groups[g] = (lo, hi - lo, rows)
        rows += hi - lo
    table = np.zeros((rows, 4), dtype=np.float32)
    for j in range(np_):
        p, (lo, _, off) = j % n, groups[j // 4]
        a = off + int(sfirst[j]) - lo
        table[a:a + int(scount[j]), j % 4] = h[p, first[p]:first[p] + count[p]]
    k_pad = int((groups[:, 0] + groups[:, 1]).max())
    qt = max(1, min(qt_max, (lds - min(k_pad, 1024)) // op + 1))
    kc = min(k_pad, (lds - (qt - 1) * op) // 8 * 8)
    return {"G": G, "groups": groups, "table": table, "qt": qt, "kc": kc, "nchunks": -(-k_pad // kc), "out_tile": qt * np_}


def resample_taps(orig_sr: int, new_sr: int = 16000, quality: str = "kaiser_best") -> dict:
    """The filter of a rate pair and quality, built once on the host in float64 and rounded once (as dft_basis()):
      o, n, width, K      the reduced ratio, the half width in input samples, taps per phase
      h (n, K) float32    h[p][k] = (base / o) sinc(pi t) w(t), t = ((k - width) n - p o) / (o n) base, 0 where |t| >= lpw
      first, count (n,)   each phase's stored band: the taps with |t| < lpw
      G, groups, table, qt, kc, nchunks      the device form (include/ultrafnd_hip.h)
      out_tile            outputs of a workgroup's tile: L.RESAMPLE_OUT_TILE (or fewer, qt) rows of G n
    orig_sr == new_sr is the one-tap filter h = [[1]]."""
    o, n = _rate_ratio(orig_sr, new_sr)
    lpw, rolloff, beta = _quality(quality)
    key = (o, n, quality)
    if key in _taps_cache:
        return _taps_cache[key]
    if o == 1 and n == 1:
        width, K = 0, 1
        h = np.ones((1, 1), dtype=np.float32)
        first, count = np.zeros(1, dtype=np.int64), np.ones(1, dtype=np.int64)
    else:
        base = min(o, n) * rolloff
        width = int(np.ceil(lpw * o / base))
        K = 2 * width + o
        num = (np.arange(K, dtype=np.int64)[None, :] - width) * n - np.arange(n, dtype=np.int64)[:, None] * o      # exact
        t = num.astype(np.float64) / float(o * n) * base
        inside = np.abs(t) < lpw
        tc = np.where(inside, t, 0.0)
        if beta is None:
            win = np.cos(np.pi * tc / (2.0 * lpw)) ** 2
        else:
            win = np.i0(beta * np.sqrt(1.0 - (tc / lpw) ** 2)) / np.i0(beta)
        h = np.where(inside, (base / o) * np.sinc(tc) * win, 0.0).astype(np.float32)      # (np.sinc(x) = sin(pi x) / (pi x))
        first = inside.argmax(axis=1).astype(np.int64)
        count = inside.sum(axis=1).astype(np.int64)
    taps = {"orig_sr": int(orig_sr), "new_sr": int(new_sr), "quality": quality, "o": o, "n": n, "width": width, "K": K, "h": h, "first": first,
            "count": count}
    taps.update(_device_table(h, first, count, o, n, K))
    _taps_cache[key] = taps
    return taps


def _taps_on(dev: torch.device, taps: dict):
    """The device tables of a filter on `dev`: uploaded once per device."""
    key = (taps["o"], taps["n"], taps["quality"], dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _taps_dev_cache:
        _taps_dev_cache[key] = (torch.from_numpy(taps["table"]).to(dev), torch.from_numpy(taps["groups"]).to(dev))
    return _taps_dev_cache[key]


@torch.no_grad()
def resample(waves: torch.Tensor, lengths=None, orig_sr: Optional[int] = None, new_sr: int = 16000, quality: str = "kaiser_best",
             scale: float = 1.0) -> dict:
    """Mono mix and sample-rate conversion of a batch, in one launch: {"waves": (B, m_max) fp32, zeros from a clip's own length on,
    "lengths": (B,) int32 = resampled_length(len_b), written on the device}, m_max = resampled_length(n_max).
    waves: (B, n_max) or (B, C, n_max) on a HIP device, fp32 or int16, ANY strides (a channel-last decoder buffer viewed as
    (B, C, n_max) is read in place).  Channels are converted to fp32, summed in index order, divided by C, multiplied by `scale`
    (1 / 32768 for PCM): NumPy's astype(float32).mean(axis=0), bit for bit.  lengths: (B,) samples per clip (a device tensor is
    not read on the host: nothing here synchronises); nothing at or past a clip's length is read.
    Every output is one fmaf chain from zero over its phase's taps in ascending tap order: the same bits alone, in any batch, in any
    row and from run to run.  A non-finite sample INSIDE a clip may poison outputs a few taps beyond its true support (the
    device table pads bands with zero taps); finite samples are unaffected."""
    if orig_sr is None:
        raise ValueError("orig_sr is required: the rate of `waves` in Hz")
    taps = resample_taps(orig_sr, new_sr, quality)
    if isinstance(waves, str) or not torch.is_tensor(waves):
        raise L.UltrafndHipError("waves must be a tensor on a HIP device (no CPU fallback)")
    dev = L.require_hip(waves)
    if waves.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"waves: dtype {waves.dtype} (fp32 or int16)")
    if waves.dim() not in (2, 3) or min(waves.shape) < 1:
        raise ValueError(f"waves: expected (B, n_max) or (B, C, n_max), got {tuple(waves.shape)}")
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError(f"scale={scale}: a finite factor")
    B, n_max = waves.shape[0], waves.shape[-1]
    C, sc = (waves.shape[1], waves.stride(1)) if waves.dim() == 3 else (1, 0)
    lens = None
    if lengths is not None:
        lens = lengths.to(dev, torch.int32).contiguous() if torch.is_tensor(lengths) else torch.tensor(list(lengths), dtype=torch.int32, device=dev)
        if lens.numel() != B:
            raise ValueError(f"lengths holds {lens.numel()} entries for {B} clips")
    m_max = resampled_length(n_max, orig_sr, new_sr)
    out = {"waves": torch.empty(B, m_max, dtype=torch.float32, device=dev), "lengths": torch.empty(B, dtype=torch.int32, device=dev)}
    table, groups = _taps_on(dev, taps)
    L.check(L.lib().ufnd_resample(waves.data_ptr(), L.RESAMPLE_I16 if waves.dtype == torch.int16 else L.RESAMPLE_F32, waves.stride(0), sc,
                                  waves.stride(-1), L.ptr(lens), table.data_ptr(), groups.data_ptr(), out["waves"].data_ptr(), out["lengths"].data_ptr(),
                                  B, C, n_max, taps["o"], taps["n"], taps["G"], taps["width"], groups.shape[0], table.shape[0], taps["qt"], taps["kc"],
                                  taps["nchunks"], scale, L.stream_ptr(dev)), "ufnd_resample")
    return out


_resample_batch = resample      # (cache_audio and the classes take a keyword named `resample`)


def _check_resample_keyword(resample, who: str):
    if resample is not None:
        try:
            _quality(resample)
        except ValueError:
            raise ValueError(f"resample={resample!r}: {who} takes None (16 kHz audio only) or one of {tuple(RESAMPLE_QUALITIES)}") from None
    return resample


def _to_16k(wavs: List[np.ndarray], rates: List[int], quality: str, device, max_batch: int) -> List[np.ndarray]:
    """Host mono clips at their own rates -> the same clips at 16 kHz: the clips of every other rate are grouped by rate and by
    length and resampled on the device."""
    out = list(wavs)
    for rate in sorted(set(rates)):
        if rate == 16000:
            continue
        idx = [i for i, r in enumerate(rates) if r == rate]
        for sub, batch, lens in _length_groups([wavs[i] for i in idx], max_batch):
            if batch.shape[1] == 0:
                continue
            r = _resample_batch(batch.to(device), lens, orig_sr=rate, quality=quality)
            y, m = r["waves"].cpu().numpy(), r["lengths"].cpu().numpy()
            for row, j in enumerate(sub):
                out[idx[j]] = np.ascontiguousarray(y[row, :m[row]])
    return out


def _clips_16k(waves, sr, who: str, quality, device, max_batch: int) -> List[np.ndarray]:
    """A list of clips -> host mono float32 at 16 kHz.  quality None: every clip must be 16 kHz already (refused by name).
    sr: one rate for all clips, or one per clip."""
    waves = list(waves)
    rates = [int(r) for r in sr] if isinstance(sr, (list, tuple, np.ndarray)) else [sr] * len(waves)
    if len(rates) != len(waves):
        raise ValueError(f"sr holds {len(rates)} rates for {len(waves)} clips")
    if quality is None:
        return [_mono_16k(a, r, who) for a, r in zip(waves, rates)]
    for r in rates:
        _rate_ratio(r, 16000)
    rates = [int(r) for r in rates]
    return _to_16k([_mono_16k(a, 16000, who) for a in waves], rates, quality, device, max_batch)


def _mono_16k(audio, sr: int, who: str) -> np.ndarray:
    """One clip as the reference's _ensure_mono_16k leaves it: host float32 (T,), channels averaged."""
    if isinstance(audio, str):
        raise TypeError(f"{who}: a str (text proxy) is not supported: the reference's _hash_embed uses Python's salted "
                        "hash(), so its vectors are not reproducible from run to run")
    if int(sr) != 16000:
        raise ValueError(f"sr={sr}: {who} takes 16 kHz audio (the reference resamples with librosa, which is not part of this package)")
    wav = audio.detach().cpu().numpy() if torch.is_tensor(audio) else np.asarray(audio)
    wav = wav.astype(np.float32)
    if wav.ndim == 2:      # (C, T) -> mono, as _ensure_mono_16k
        wav = wav.mean(axis=0)
    if wav.ndim != 1:
        raise ValueError(f"audio: expected (T,) or (C, T), got {wav.shape}")
    return wav


def _length_groups(wavs: List[np.ndarray], max_batch: int):
    """Clips sorted by length, in groups of at most max_batch neighbours (bounded padding): (indices, (n, n_max) zero-padded host
    batch, lengths) per group."""
    order = sorted(range(len(wavs)), key=lambda i: len(wavs[i]))
    for s0 in range(0, len(order), max_batch):
        idx = order[s0:s0 + max_batch]
        batch = torch.zeros(len(idx), max(len(wavs[i]) for i in idx))
        for r, i in enumerate(idx):
            batch[r, :len(wavs[i])] = torch.from_numpy(wavs[i])
        yield idx, batch, [len(wavs[i]) for i in idx]


def _require_stft_lengths(wavs: List[np.ndarray]) -> None:
    for w in wavs:
        if len(w) < STFT_MIN_SAMPLES:
            raise ValueError(f"clip length {len(w)}: the STFT branch needs at least {STFT_MIN_SAMPLES} samples (torch.stft's reflect padding of 200)")


def _require_samples(wavs: List[np.ndarray]) -> None:
    for w in wavs:
        if len(w) < 1:
            raise ValueError("clip length 0: the librosa branch needs at least one sample")


class SpectralForensics:
    """The reference's audio feature extractor (src/core_blocks/audio_blocks.py) on the GPU.
      branch="w2v2"  (default) its wav2vec2 branch: the encoder above.
      branch="stft"  its _torch_stft_fallback, the branch it takes without a checkpoint and without librosa: no encoder is built.
      branch="librosa"  its _librosa_spectral, the branch it takes without a checkpoint WITH librosa (spectral_descriptors: zero
                     padding, any clip of at least one sample): no encoder is built.
    resample=None refuses anything but 16 kHz audio; a quality name ("kaiser_best", ...) resamples other rates on the device first
    (audio.resample), and the minimum-length checks then apply to the resampled clip."""

    def __init__(self, dim: int = 128, encoder: Optional[Wav2Vec2AudioEncoder] = None, device="cuda", max_batch: int = 32, branch: str = "w2v2",
                 resample: Optional[str] = None):
        if branch not in ("w2v2", "stft", "librosa"):
            raise ValueError(f"branch={branch!r}: 'w2v2', 'stft' or 'librosa'")
        self.resample = _check_resample_keyword(resample, "SpectralForensics")
        self.dim, self.branch = int(dim), branch
        if self.dim < 1:
            raise ValueError(f"dim={dim}: at least 1")
        self.max_batch = int(max_batch)
        self.device = torch.device(device)
        if branch != "w2v2":
            if encoder is not None:
                raise ValueError(f"branch={branch!r} runs no encoder: pass encoder=None")
            self.encoder = None
            return
        self.encoder = encoder if encoder is not None else Wav2Vec2AudioEncoder(out_dim=self.dim).to(device)
        if self.encoder.out_dim != self.dim:
            raise ValueError(f"dim={self.dim} but the encoder projects to {self.encoder.out_dim}")

    @staticmethod
    def _mono_16k(audio, sr: int) -> np.ndarray:
        return _mono_16k(audio, sr, "SpectralForensics")

    def extract(self, audio_or_text, sr: int = 16000) -> np.ndarray:
        """One clip -> (dim,) float32."""
        wav = _clips_16k([audio_or_text], sr, "SpectralForensics", self.resample, self.device, self.max_batch)[0]
        if self.branch == "stft":
            _require_stft_lengths([wav])
            return stft_forensics(torch.from_numpy(wav)[None].to(self.device), None, self.dim)["features"].cpu().numpy()[0]
        if self.branch == "librosa":
            _require_samples([wav])
            return spectral_descriptors(torch.from_numpy(wav)[None].to(self.device), None, self.dim)["features"].cpu().numpy()[0]
        return self.encoder(torch.from_numpy(wav)[None]).cpu().numpy()[0]

    def extract_batch(self, waves, sr: int = 16000) -> np.ndarray:
        """A list of clips -> (N, dim) float32: the batched entry of a cache builder.  Clips are sorted by length and run in groups
        of at most max_batch neighbours, which bounds the padding; every row equals extract() of its clip bit for bit.
        sr: one rate for all clips, or one per clip (with resample set)."""
        wavs = _clips_16k(waves, sr, "SpectralForensics", self.resample, self.device, self.max_batch)
        if self.branch == "stft":
            _require_stft_lengths(wavs)
        if self.branch == "librosa":
            _require_samples(wavs)
        out = np.zeros((len(wavs), self.dim), dtype=np.float32)
        for idx, batch, lens in _length_groups(wavs, self.max_batch):
            if self.branch == "stft":
                out[idx] = stft_forensics(batch.to(self.device), lens, self.dim)["features"].cpu().numpy()
            elif self.branch == "librosa":
                out[idx] = spectral_descriptors(batch.to(self.device), lens, self.dim)["features"].cpu().numpy()
            else:
                out[idx] = self.encoder(batch, lens).cpu().numpy()
        return out


class MelSpectrogramGenerator:
    """MelSpectrogramGenerator of the reference.
      branch="torch"    (default) its branch without librosa: the STFT magnitudes' bins 3m, 3m + 1, 3m + 2 averaged into 64 bands
                        ([band, time]; bins 192 .. 200 are dropped); clips of at least 201 samples.
      branch="librosa"  its branch with librosa: the (64, T) mel spectrogram in dB (mel_spectrogram: zero padding, Slaney scale and
                        norm, ref = the clip's maximum, floor -80; T = 1 + len // 160); any clip of at least one sample.  htk, norm
                        and pad_mode name what that branch is built for; any other value is refused.
    The reference's geometry only; anything else is refused by name."""

    def __init__(self, sr: int = 16000, n_mels: int = N_BANDS, n_fft: int = N_FFT, hop_length: int = HOP, device="cuda", max_batch: int = 32,
                 resample: Optional[str] = None, branch: str = "torch", htk: bool = False, norm: Optional[str] = "slaney",
                 pad_mode: str = "constant"):
        self.resample = _check_resample_keyword(resample, "MelSpectrogramGenerator")
        for name, got, want in (("sr", sr, 16000), ("n_mels", n_mels, N_BANDS), ("n_fft", n_fft, N_FFT), ("hop_length", hop_length, HOP)):
            if int(got) != want:
                raise ValueError(f"{name}={got!r}: MelSpectrogramGenerator is built for the reference's defaults ({name}={want})")
        if branch not in ("torch", "librosa"):
            raise ValueError(f"branch={branch!r}: 'torch' or 'librosa'")
        for name, got, want in (("htk", htk, False), ("norm", norm, "slaney"), ("pad_mode", pad_mode, "constant")):
            if got != want or type(got) is not type(want):
                raise ValueError(f"{name}={got!r}: only {name}={want!r} is built (the librosa branch's Slaney scale and norm, zero padding; "
                                 "branch='torch' takes none of the three)")
        self.sr, self.n_mels, self.n_fft, self.hop, self.branch = 16000, N_BANDS, N_FFT, HOP, branch
        self.device, self.max_batch = torch.device(device), int(max_batch)

    def generate_batch(self, waves, sr: int = 16000, flatten: bool = True) -> List[np.ndarray]:
        """A list of clips -> per clip the (64, T_b) float32 matrix, or its flattening."""
        wavs = _clips_16k(waves, sr, "MelSpectrogramGenerator", self.resample, self.device, self.max_batch)
        if self.branch == "librosa":
            _require_samples(wavs)
        else:
            _require_stft_lengths(wavs)
        out: List[Optional[np.ndarray]] = [None] * len(wavs)
        for idx, batch, lens in _length_groups(wavs, self.max_batch):
            if self.branch == "librosa":
                mel, frames = mel_spectrogram(batch.to(self.device), lens)["mel_db"].cpu().numpy(), mel_frame_count
            else:
                mel, frames = stft_forensics(batch.to(self.device), lens, want=("mel_like",))["mel_like"].cpu().numpy(), stft_frame_count
            for r, i in enumerate(idx):
                m = np.ascontiguousarray(mel[r, :, :frames(lens[r])])
                out[i] = m.flatten() if flatten else m
        return out

    def generate(self, wave, sr: int = 16000, flatten: bool = True) -> np.ndarray:
        return self.generate_batch([wave], sr, flatten)[0]


class VoiceCloneDetector:
    """VoiceCloneDetector of the reference.
      branch="energy"   (default) its energy branch: e = mean(x^2), score = clip(e / (e + 1), 0, 1).
      branch="librosa"  its librosa descriptor mix (spectral_descriptors' clone_score)."""

    def __init__(self, device="cuda", max_batch: int = 32, resample: Optional[str] = None, branch: str = "energy"):
        if branch not in ("energy", "librosa"):
            raise ValueError(f"branch={branch!r}: 'energy' or 'librosa'")
        self.branch = branch
        self.device, self.max_batch = torch.device(device), int(max_batch)
        self.resample = _check_resample_keyword(resample, "VoiceCloneDetector")

    def score_batch(self, waves, sr: int = 16000) -> np.ndarray:
        """A list of clips -> (N,) float32 scores; every entry equals score() of its clip bit for bit."""
        wavs = _clips_16k(waves, sr, "VoiceCloneDetector", self.resample, self.device, self.max_batch)
        out = np.zeros(len(wavs), dtype=np.float32)
        for idx, batch, lens in _length_groups(wavs, self.max_batch):
            if batch.shape[1] == 0:      # (empty clips only: the mean of nothing; the reference returns NaN there, this returns 0)
                continue
            if self.branch == "librosa":
                out[idx] = spectral_descriptors(batch.to(self.device), lens, want=("clone_score",))["clone_score"].cpu().numpy()
                continue
            out[idx] = wave_energy(batch.to(self.device), lens)["score"].cpu().numpy()
        return out

    def score(self, audio_or_text, sr: int = 16000) -> float:
        return float(self.score_batch([audio_or_text], sr)[0])


@torch.no_grad()
def cache_audio(waves: torch.Tensor, lengths=None, audio_dim: int = 128, sr: int = 16000, resample: str = "kaiser_best",
                branch: str = "stft") -> torch.Tensor:
    """The `audio` row of the reference's cache builder on real waveforms, on a branch the reference takes without a checkpoint:
    SpectralForensics(dim=audio_dim).extract of every clip, (B, audio_dim) fp32 on the waves' device (a vector of unit norm already).
    branch="stft" (default): the branch of a host without librosa; branch="librosa": the 11-descriptor branch of a host with it.
    sr != 16000: the clips are mixed to mono and resampled on the device first (audio.resample at quality `resample`, fp32 or int16
    input, any strides); sr == 16000 is the direct path."""
    if branch not in ("stft", "librosa"):
        raise ValueError(f"branch={branch!r}: 'stft' or 'librosa'")
    entry = stft_forensics if branch == "stft" else spectral_descriptors
    _rate_ratio(sr, 16000)
    if int(sr) == 16000:
        return entry(waves, lengths, audio_dim)["features"]
    _quality(resample)
    r = _resample_batch(waves, lengths, orig_sr=sr, quality=resample)
    return entry(r["waves"], r["lengths"], audio_dim)["features"]
