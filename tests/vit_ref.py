"""TEST INFRASTRUCTURE for ultrafnd_git_amd/encoders.py: ClipVisualEncoder (CPU, float64).

  reference(sd, frames, heads)  the yardstick: oracle/encoders_ref (vit_pooled / visual_features) on float64 weights; the installed
                                transformers.CLIPVisionModelWithProjection in float64 pins it (tests/test_vit_ref.py, hf_model below).
  mirror(sd, frames, ...)       the same arithmetic written out in float64 torch, with operands rounded to bf16 exactly where the
                                product rounds them (bf16=True), in the encoder's three forms (FORMS):
                                  every form   the patch panel and the patch weight, q / k / v, the attention probabilities before
                                               P V, ctx, the quick-GELU output, the pooled post_layernorm row, every GEMM weight
                                  unfolded     a LayerNorm's consumer reads the rounded LayerNorm output
                                  folded       it reads the rounded UN-normalised stream against the rounded W * gamma, normalised
                                               with the statistics of the unrounded row
                                  folded-bf16  the rounding IS the stream: a residual GEMM adds its product to the rounded row
                                The LayerNorm / softmax statistics, the class token + position sum, the fp32 sums a hidden state is
                                read from and the L2 normalisations stay unrounded.  With bf16=False it is the yardstick itself.

Both return the same dict of checkpoints: "embed" (N, T, H: pre_layrnorm's output, hidden_states[0]), "layers" [hidden_states[1], ...],
"pooled" (N, H: post_layernorm of the class rows, as the projection reads it), "image_embeds" (N, P), "feature" (B, P: per frame
x / (||x|| + 1e-9), for several frames their mean, normalised again).  frames: (B, F, 3, S, S); N = B F.

Bounds: tests/audio_ref.py's convention (criteria / bounds_from_mirror / MIRROR_SANITY).
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from oracle import encoders_ref as E
from tests.audio_ref import BF16_U, BOUND_FACTOR, EPS32, MIRROR_SANITY, bounds_from_mirror, criteria, mirror_within_sanity  # noqa: F401

FORMS = {"folded-bf16": (True, "bf16"), "folded-fp32": (True, "fp32"), "unfolded": (False, "fp32")}


def case_weights(sd: Dict[str, torch.Tensor], seed: int = 31) -> Dict[str, torch.Tensor]:
    """The tests' weights from an encoder's seeded state_dict: a non-trivial affine everywhere (the constructor leaves gamma = 1,
    beta = 0, bias = 0)."""
    sd = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        if ("layer_norm" in k or "layernorm" in k or "layrnorm" in k) and k.endswith(".weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
    return sd


def make_frames(B: int, Fr: int, image: int, seed: int = 0) -> torch.Tensor:
    """(B, F, 3, S, S) fp32: seeded noise around a per-channel offset, of the preprocessed pixels' order of magnitude."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Fr, 3, image, image, generator=g) + torch.tensor([0.3, -0.2, 0.1])[None, None, :, None, None]


def hf_model(sd: Dict[str, torch.Tensor], layers: int, hidden: int, heads: int, inter: int, patch: int, image: int, proj: int):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(hidden_size=hidden, intermediate_size=inter, projection_dim=proj, num_hidden_layers=layers, num_attention_heads=heads,
                           image_size=image, patch_size=patch, hidden_act="quick_gelu", layer_norm_eps=1e-5, attention_dropout=0.0)
    cfg._attn_implementation = "eager"
    m = CLIPVisionModelWithProjection(cfg).double().eval()
    missing, unexpected = m.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
    assert set(missing) <= {"vision_model.embeddings.position_ids"} and not unexpected, (missing, unexpected)
    return m


def _l2n(x: torch.Tensor) -> torch.Tensor:
    return x / (x.norm(dim=-1, keepdim=True) + 1e-9)


def _features(e: torch.Tensor, B: int, Fr: int) -> torch.Tensor:
    e = _l2n(e).view(B, Fr, -1)
    return e[:, 0] if Fr == 1 else _l2n(e.mean(dim=1))


@torch.no_grad()
def hf_reference(model, frames: torch.Tensor) -> dict:
    B, Fr = frames.shape[:2]
    out = model(pixel_values=frames.reshape(B * Fr, *frames.shape[2:]).double(), output_hidden_states=True)
    hs = out.hidden_states
    pooled = model.vision_model.post_layernorm(out.last_hidden_state[:, 0])
    return {"embed": hs[0], "layers": list(hs[1:]), "pooled": pooled, "image_embeds": out.image_embeds, "feature": _features(out.image_embeds, B, Fr)}


@torch.no_grad()
def reference(sd: Dict[str, torch.Tensor], frames: torch.Tensor, heads: int) -> dict:
    w = {k: v.double() for k, v in sd.items()}
    B, Fr = frames.shape[:2]
    col: dict = {}
    pooled = E.vit_pooled(w, frames.reshape(B * Fr, *frames.shape[2:]).double(), heads, collect=col)
    e = pooled @ w["visual_projection.weight"].T
    layers = [col[k] for k in sorted(col) if k > 0]
    return {"embed": col[0], "layers": layers, "pooled": pooled, "image_embeds": e, "feature": E.visual_features(w, frames.double(), heads)}


def _rb(t: torch.Tensor, on: bool) -> torch.Tensor:
    return t.to(torch.bfloat16).double() if on else t


@torch.no_grad()
def mirror(sd: Dict[str, torch.Tensor], frames: torch.Tensor, layers: int, heads: int, bf16: bool = True, form: str = "folded-bf16",
           eps: float = 1e-5) -> dict:
    fold, stream = FORMS[form]
    fold, sb = fold and bf16, (stream == "bf16") and bf16
    w = {k: v.double() for k, v in sd.items()}
    V = "vision_model."
    B, Fr = frames.shape[:2]
    N = B * Fr
    pw = w[V + "embeddings.patch_embedding.weight"]
    H, patch = pw.shape[0], pw.shape[-1]
    pe = F.conv2d(_rb(frames.reshape(N, *frames.shape[2:]).double(), bf16), _rb(pw, bf16), stride=patch).flatten(2).transpose(1, 2)
    x = torch.cat([w[V + "embeddings.class_embedding"].expand(N, 1, H), pe], dim=1) + w[V + "embeddings.position_embedding.weight"][None]
    x = F.layer_norm(x, (H,), w[V + "pre_layrnorm.weight"], w[V + "pre_layrnorm.bias"], eps)
    embed = x.clone()
    T = x.shape[1]

    def lin(a, name):
        return _rb(a, bf16) @ _rb(w[name + ".weight"], bf16).T + w[name + ".bias"]

    def lin_ln(y, ln_name, name):      # Linear(LayerNorm(y))
        if not fold:
            return lin(F.layer_norm(y, (H,), w[ln_name + ".weight"], w[ln_name + ".bias"], eps), name)
        mu, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
        n = (_rb(y, True) - mu) / torch.sqrt(var + eps)
        W = w[name + ".weight"]
        return n @ _rb(W * w[ln_name + ".weight"][None, :], True).T + (w[name + ".bias"] + W @ w[ln_name + ".bias"])

    hs = []
    for i in range(layers):
        P = V + f"encoder.layers.{i}."
        q, k, v = (_rb(lin_ln(x, P + "layer_norm1", P + f"self_attn.{n}"), bf16).view(N, T, heads, 64).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        p = torch.softmax(q @ k.transpose(2, 3) * 0.125, dim=-1)
        ctx = _rb((_rb(p, bf16) @ v).transpose(1, 2).reshape(N, T, H), bf16)
        x = _rb(x, sb) + lin(ctx, P + "self_attn.out_proj")
        a = lin_ln(x, P + "layer_norm2", P + "mlp.fc1")
        x = _rb(x, sb) + lin(_rb(a * torch.sigmoid(1.702 * a), bf16), P + "mlp.fc2")
        hs.append(x.clone())      # hidden_states[i + 1], as hidden_state(n_layers = i + 1) reads it: the fp32 sums of the last layer run
    pooled = _rb(F.layer_norm(x[:, 0], (H,), w[V + "post_layernorm.weight"], w[V + "post_layernorm.bias"], eps), bf16)
    e = pooled @ _rb(w["visual_projection.weight"], bf16).T
    return {"embed": embed, "layers": hs, "pooled": pooled, "image_embeds": e, "feature": _features(e, B, Fr)}
