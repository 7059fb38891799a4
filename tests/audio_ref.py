"""TEST INFRASTRUCTURE for ultrafnd_git_amd/audio.py (CPU, float64).

  reference(sd, wave, layers)   the yardstick: the installed transformers.Wav2Vec2Model in float64 with
                                Wav2Vec2FeatureExtractor() for the normalisation, run ONE CLIP AT A TIME, the way
                                SpectralForensics._w2v2_features calls it (src/core_blocks/audio_blocks.py:131-139).
  mirror(sd, wave, layers)      the same arithmetic written out in float64 torch, with operands rounded to bf16 exactly where the
                                product rounds them (bf16=True): the conv / GEMM weights, every conv / GEMM A operand (conv
                                layers 1-6, the feature projection, the positional conv, the four Linears of a layer), q / k / v,
                                the attention probabilities before P V, and ctx.  Statistics, residuals, LayerNorm / GroupNorm /
                                softmax and the fp32-only stages stay unrounded.  With bf16=False it is the yardstick itself
                                (tests/test_audio_ref.py holds it to HF).

Both return the same dict of checkpoints: "norm" (n,), "conv0" (T1, 512), "conv" (T, 512), "pos" (T, 768),
"layers" [hidden_states[1], ...] each (T, 768), "feature" (out_dim,).

Bounds.  Every comparison of the GPU against float64 is held to BOUND_FACTOR x the mirror's own error against float64 on that same
input, per criterion (criteria()); the bound never comes from the code under test.  fp32-only stages: FP32_BOUNDS.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F

CONV_KERNELS = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDES = (5, 2, 2, 2, 2, 2, 2)
BOUND_FACTOR = 3.0          # the upper end of the 2-3 x the README states for the other encoders (summation order is not mirrored)
BF16_U = 2.0 ** -9          # bf16 unit roundoff
# The input condition: on every input the tests use, the mirror's own error against float64 stays within these multiples of the bf16
# unit roundoff (max-abs relative to the largest |reference| of the stage).  Five to six roundings in sequence reach 3-5 u; an input
# on which the reference alone left this band would make "3 x the mirror" mean nothing.
MIRROR_SANITY = {"max_abs": 16 * BF16_U, "rel_l2": 8 * BF16_U, "one_minus_cos": (8 * BF16_U) ** 2 / 2}
EDGE_LENGTHS = (400, 719, 720, 1040, 16000, 41360, 41680)
FRAMES = {400: 1, 719: 1, 720: 2, 16000: 49, 41360: 129, 41680: 130}

EPS32 = 2.0 ** -24          # fp32 unit roundoff
# fp32-only stages: bounds from rounding, relative to the largest magnitude of the float64 result (max-abs / max|ref|).
#   norm     (x - mean) * inv: mean and inv carry a few ulp each (float64 combine of fp32 partials), one subtraction, one product:
#            <= 8 eps relative to the largest sample
#   conv0    a 10-term fma chain, GroupNorm statistics over the clip's frames from fp32 partials combined in float64 (a few eps
#            of the normalised value), the affine map, and an erf-GELU whose erf is good to 1.5e-7 (0.75e-7 |x| on the output):
#            <= (64 eps + 0.75e-7) of the largest value
#   pool     a mean over T <= 130 fp32 rows in a fixed tree: <= (T + 2) eps of the largest |hidden|, bounded with T = 130
#   proj     a 768-term fma chain on the pooled row (+ bias): <= 770 eps of sum_k |w_k x_k| + |b| (the test computes that scale)
FP32_BOUNDS = {"norm": 8 * EPS32, "conv0": 64 * EPS32 + 0.75e-7, "pool": 132 * EPS32, "proj": 770 * EPS32}


def frame_counts(n: int) -> List[int]:
    out, t = [], int(n)
    for k, s in zip(CONV_KERNELS, CONV_STRIDES):
        t = (t - k) // s + 1
        out.append(t)
    return out


def criteria(got, ref) -> Dict[str, float]:
    """The project's three criteria of `got` against `ref` (float64): max-abs, relative L2, 1 - cosine."""
    g = torch.as_tensor(got).double().flatten()
    r = torch.as_tensor(ref).double().flatten()
    d = g - r
    rn, gn = r.norm(), g.norm()
    cos = float((g @ r) / (gn * rn)) if float(gn) > 0 and float(rn) > 0 else 1.0
    return {"max_abs": float(d.abs().max()), "rel_l2": float(d.norm() / rn) if float(rn) > 0 else float(d.norm()), "one_minus_cos": max(0.0, 1.0 - cos)}


def bounds_from_mirror(mirror_out, ref_out) -> Dict[str, float]:
    """BOUND_FACTOR x the mirror's own error on this input, per criterion.  Used for stages that carry bf16 roundings only (the
    mirror's error is positive there: tests/test_audio_ref.py); fp32-only stages have FP32_BOUNDS."""
    return {k: BOUND_FACTOR * v for k, v in criteria(mirror_out, ref_out).items()}


def mirror_within_sanity(mirror_out, ref_out) -> Dict[str, tuple]:
    """The criteria on which the mirror leaves MIRROR_SANITY on this input ({} = the input is admissible)."""
    c = criteria(mirror_out, ref_out)
    scale = float(torch.as_tensor(ref_out).double().abs().max())
    cap = dict(MIRROR_SANITY, max_abs=MIRROR_SANITY["max_abs"] * scale)
    return {k: (c[k], cap[k]) for k in c if not 0 < c[k] <= cap[k]}


# the inputs of tests/test_gpu_audio.py (tests/test_audio_ref.py holds every one of them to MIRROR_SANITY)
# 400: one frame (GroupNorm over 79 conv0 frames, a one-frame transformer); 645: S1 = 128 hit exactly; 719 / 720: the floor in the
# frame count; 1,040: 3 frames; 9,999: a ragged slab; 16,000: 49 frames (positional conv all-edge); 41,360 / 41,680: 129 / 130 frames
# (one / two interior tap windows)
LENGTHS = (400, 645, 719, 720, 1040, 9999, 16000, 41360, 41680)
MIXED = (400, 16000, 9999, 41680)
OUTLIER_CHANNEL, OUTLIER_LENGTHS = 5, (1040, 16000)
FULL_DEPTH_SEEDS = (100, 101)      # two 16,000-sample clips through 12 layers


def case_weights(sd: Dict[str, torch.Tensor], scale_channel=None) -> Dict[str, torch.Tensor]:
    """The tests' weights from an encoder's seeded state_dict: a non-trivial affine everywhere (the constructor leaves gamma = 1,
    beta = 0, bias = 0) and, with scale_channel, that conv0 channel's weight scaled 20 x."""
    sd = {k: v.clone() for k, v in sd.items()}
    if scale_channel is not None:
        sd["feature_extractor.conv_layers.0.conv.weight"][scale_channel] *= 20.0
    g = torch.Generator().manual_seed(7)
    for k, v in sd.items():
        if k.endswith("layer_norm.weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
    return sd


def make_waves(lengths, seed: int = 0) -> List[torch.Tensor]:
    """Seeded speech-like clips (a few decaying sinusoids + noise, a DC offset and an amplitude well off 1, so that the
    normalisation matters), fp32."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lengths:
        t = torch.arange(n, dtype=torch.float64) / 16000.0
        x = torch.zeros(n, dtype=torch.float64)
        for _ in range(4):
            f0 = 80.0 + 3000.0 * float(torch.rand((), generator=g))
            x += float(torch.rand((), generator=g)) * torch.sin(2 * np.pi * f0 * t + 6.28 * float(torch.rand((), generator=g)))
        x += 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
        out.append((0.05 * x + 0.02).float())
    return out


def _rb(t: torch.Tensor, on: bool) -> torch.Tensor:
    return t.to(torch.bfloat16).double() if on else t


def hf_model(sd: Dict[str, torch.Tensor], layers: int):
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    cfg = Wav2Vec2Config(num_hidden_layers=layers)
    cfg._attn_implementation = "eager"
    m = Wav2Vec2Model(cfg).double().eval()
    own = {k: v.double() for k, v in sd.items() if not k.startswith("proj.")}
    missing, unexpected = m.load_state_dict(own, strict=False)
    assert set(missing) <= {"masked_spec_embed"} and not unexpected, (missing, unexpected)
    return m


@torch.no_grad()
def reference(sd: Dict[str, torch.Tensor], wave: torch.Tensor, layers: int, model=None) -> dict:
    from transformers import Wav2Vec2FeatureExtractor
    m = model if model is not None else hf_model(sd, layers)
    # (the extractor's __call__ casts to float32 first; its normalisation routine itself keeps the float64 it is given)
    x = torch.from_numpy(Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm([wave.double().numpy()], None)[0])[None]
    assert Wav2Vec2FeatureExtractor().do_normalize and x.dtype == torch.float64
    norm = x[0].clone()
    keep = {}
    h = m.feature_extractor.conv_layers[0].register_forward_hook(lambda mod, i, o: keep.__setitem__("conv0", o[0].T.clone()))
    try:
        out = m(x, output_hidden_states=True)
    finally:
        h.remove()
    hs = out.hidden_states
    feat = out.last_hidden_state.mean(dim=1)[0] @ sd["proj.weight"].double().T + sd["proj.bias"].double()
    return {"norm": norm, "conv0": keep["conv0"], "conv": m.feature_extractor(x)[0].T.clone(), "pos": hs[0][0], "layers": [t[0] for t in hs[1:]],
            "feature": feat}


@torch.no_grad()
def mirror(sd: Dict[str, torch.Tensor], wave: torch.Tensor, layers: int, bf16: bool = True, heads: int = 12, eps: float = 1e-5) -> dict:
    w = {k: v.double() for k, v in sd.items()}
    Fx, E = "feature_extractor.conv_layers.", "encoder."
    x = wave.double()
    norm = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
    h = F.conv1d(norm[None, None], w[Fx + "0.conv.weight"], stride=CONV_STRIDES[0])
    h = F.gelu(F.group_norm(h, 512, w[Fx + "0.layer_norm.weight"], w[Fx + "0.layer_norm.bias"], eps))
    conv0 = h[0].T.clone()
    for i in range(1, 7):
        h = F.gelu(F.conv1d(_rb(h, bf16), _rb(w[Fx + f"{i}.conv.weight"], bf16), stride=CONV_STRIDES[i]))
    conv = h[0].T.clone()                                   # (T, 512): layer 6 stays fp32 in the product
    f = F.layer_norm(conv, (512,), w["feature_projection.layer_norm.weight"], w["feature_projection.layer_norm.bias"], eps)
    x0 = _rb(f, bf16) @ _rb(w["feature_projection.projection.weight"], bf16).T + w["feature_projection.projection.bias"]
    v = w[E + "pos_conv_embed.conv.parametrizations.weight.original1"]
    g = w[E + "pos_conv_embed.conv.parametrizations.weight.original0"]
    if bf16:      # the product resolves the parametrisation in fp32, then rounds
        pw = (g.float() * v.float() / v.float().norm(p=2, dim=(0, 1), keepdim=True)).double()
    else:
        pw = g * v / v.norm(p=2, dim=(0, 1), keepdim=True)
    pc = F.conv1d(_rb(x0, bf16).T[None], _rb(pw, bf16), w[E + "pos_conv_embed.conv.bias"], padding=64, groups=16)[0, :, :-1].T
    hcur = F.layer_norm(x0 + F.gelu(pc), (768,), w[E + "layer_norm.weight"], w[E + "layer_norm.bias"], eps)
    pos = hcur.clone()
    T, hs = hcur.shape[0], []

    def lin(a, name):
        return _rb(a, bf16) @ _rb(w[name + ".weight"], bf16).T + w[name + ".bias"]

    for i in range(layers):
        P = E + f"layers.{i}."
        q, k, vv = (_rb(lin(hcur, P + f"attention.{n}"), bf16).view(T, heads, 64).transpose(0, 1) for n in ("q_proj", "k_proj", "v_proj"))
        p = torch.softmax(q @ k.transpose(1, 2) * 0.125, dim=-1)
        ctx = _rb((_rb(p, bf16) @ vv).transpose(0, 1).reshape(T, heads * 64), bf16)
        h1 = F.layer_norm(hcur + lin(ctx, P + "attention.out_proj"), (768,), w[P + "layer_norm.weight"], w[P + "layer_norm.bias"], eps)
        ff = lin(_rb(F.gelu(lin(h1, P + "feed_forward.intermediate_dense")), bf16), P + "feed_forward.output_dense")
        hcur = F.layer_norm(h1 + ff, (768,), w[P + "final_layer_norm.weight"], w[P + "final_layer_norm.bias"], eps)
        hs.append(hcur.clone())
    feat = hcur.mean(dim=0) @ w["proj.weight"].T + w["proj.bias"]
    return {"norm": norm, "conv0": conv0, "conv": conv, "pos": pos, "layers": hs, "feature": feat}


# ---- the overlapping-row formulation on the CPU (float64): what the slab arithmetic of the product computes
def conv_rows(a_rows: torch.Tensor, w_tap_major: torch.Tensor, M: int, lda: int) -> torch.Tensor:
    """Output row r = W . flat(A)[r lda : r lda + K]: the GEMM with an overlapping-row A operand (no activation)."""
    K = w_tap_major.shape[1]
    flat = a_rows.reshape(-1)
    idx = (torch.arange(M)[:, None] * lda + torch.arange(K)[None, :])
    return flat[idx] @ w_tap_major.T
