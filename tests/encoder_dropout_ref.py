"""Float64 autograd restatement of the two trainable encoders WITH train-mode dropout (tests only).

oracle/encoders_ref.py restates BertModel / CLIPVisionModel without dropout (the reference keeps them frozen).  This module repeats
its arithmetic operation for operation and multiplies explicit masks in at HF's five dropout sites:

  site        text / vision   HF module                          tensor dropped                                   tag
  emb         text            BertEmbeddings.dropout             LayerNorm(word + pos + type)                     256
  attn i      both            eager_attention_forward            softmax probabilities, before @ V                257 + 3i / 4096 + i
  attn_out i  text            BertSelfOutput.dropout             dense(ctx) + bias, before + residual, LayerNorm  258 + 3i
  ffn_out i   text            BertOutput.dropout                 dense(gelu(..)) + bias, likewise                 259 + 3i

With masks=None every function here equals its oracle.encoders_ref counterpart (tests/test_encoder_dropout_ref.py).

The masks are built from tests/dropout_mirror.py with the kernels' element numbering (include/ultrafnd_hip.h, ufnd_dropout):
attention probabilities ((b heads + h) L + q) Lp + k with Lp = L rounded up to 4; hidden states row H + col.  The tags restate
csrc/common.hpp's ranges; they are not imported from the package, so a wrong tag there shows up as a mismatch here.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import encoders_ref as E
from tests import dropout_mirror as DM

TAG_TEXT_EMB = 256


def tag_text(layer: int, site: str) -> int:
    return 257 + 3 * layer + {"attn": 0, "attn_out": 1, "ffn_out": 2}[site]


def tag_vision(layer: int) -> int:
    return 4096 + layer


def attention_mask_multipliers(seed: int, step: int, tag: int, p: float, N: int, heads: int, L: int) -> torch.Tensor:
    """(N, heads, L, L) float32 multipliers of the softmax probabilities: element (n, h, q, k) is ((n heads + h) L + q) Lp + k."""
    lp = (L + 3) // 4 * 4
    return torch.from_numpy(DM.multipliers(seed, step, tag, p, N * heads * L, L, lp)).view(N, heads, L, L)


def hidden_multipliers(seed: int, step: int, tag: int, p: float, N: int, L: int, H: int) -> torch.Tensor:
    """(N, L, H) float32 multipliers of a hidden-state site: element (row = n L + l, col) is row H + col."""
    return torch.from_numpy(DM.multipliers(seed, step, tag, p, N * L, H, H)).view(N, L, H)


def text_masks(seed: int, step: int, B: int, L: int, layers: int, heads: int = 12, hidden: int = 768,
               p_hidden: float = 0.1, p_attn: float = 0.1) -> Dict:
    m = {"emb": hidden_multipliers(seed, step, TAG_TEXT_EMB, p_hidden, B, L, hidden)}
    for i in range(layers):
        m[("attn", i)] = attention_mask_multipliers(seed, step, tag_text(i, "attn"), p_attn, B, heads, L)
        m[("attn_out", i)] = hidden_multipliers(seed, step, tag_text(i, "attn_out"), p_hidden, B, L, hidden)
        m[("ffn_out", i)] = hidden_multipliers(seed, step, tag_text(i, "ffn_out"), p_hidden, B, L, hidden)
    return m


def vision_masks(seed: int, step: int, N: int, T: int, layers: int, heads: int = 12, p_attn: float = 0.1) -> Dict:
    return {("attn", i): attention_mask_multipliers(seed, step, tag_vision(i), p_attn, N, heads, T) for i in range(layers)}


def _mul(x: torch.Tensor, masks: Optional[Dict], key) -> torch.Tensor:
    if masks is None or key not in masks:
        return x
    return x * masks[key].to(x.dtype)


# --------------------------------------------------------------------------
def _mha(x, wq, bq, wk, bk, wv, bv, heads: int, add_mask, pmask):
    B, L, H = x.shape
    d = H // heads
    q = F.linear(x, wq, bq).view(B, L, heads, d).transpose(1, 2)
    k = F.linear(x, wk, bk).view(B, L, heads, d).transpose(1, 2)
    v = F.linear(x, wv, bv).view(B, L, heads, d).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * (d ** -0.5)
    if add_mask is not None:
        s = s + add_mask
    p = torch.softmax(s, dim=-1)
    if pmask is not None:
        p = p * pmask.to(p.dtype)
    return (p @ v).transpose(1, 2).reshape(B, L, H)


def bert_last_hidden_state(w, input_ids, attention_mask, heads: int = 12, eps: float = 1e-12, masks: Optional[Dict] = None):
    B, L = input_ids.shape
    H = w["embeddings.word_embeddings.weight"].shape[1]
    x = (w["embeddings.word_embeddings.weight"][input_ids]
         + w["embeddings.position_embeddings.weight"][:L][None]
         + w["embeddings.token_type_embeddings.weight"][0][None, None])
    x = F.layer_norm(x, (H,), w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], eps)
    x = _mul(x, masks, "emb")
    add_mask = (1.0 - attention_mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    i = 0
    while f"encoder.layer.{i}.attention.self.query.weight" in w:
        P = f"encoder.layer.{i}."
        ctx = _mha(x, w[P + "attention.self.query.weight"], w[P + "attention.self.query.bias"],
                   w[P + "attention.self.key.weight"], w[P + "attention.self.key.bias"],
                   w[P + "attention.self.value.weight"], w[P + "attention.self.value.bias"],
                   heads, add_mask, None if masks is None else masks.get(("attn", i)))
        y = _mul(F.linear(ctx, w[P + "attention.output.dense.weight"], w[P + "attention.output.dense.bias"]), masks, ("attn_out", i))
        x = F.layer_norm(y + x, (H,), w[P + "attention.output.LayerNorm.weight"], w[P + "attention.output.LayerNorm.bias"], eps)
        h = F.gelu(F.linear(x, w[P + "intermediate.dense.weight"], w[P + "intermediate.dense.bias"]))
        y = _mul(F.linear(h, w[P + "output.dense.weight"], w[P + "output.dense.bias"]), masks, ("ffn_out", i))
        x = F.layer_norm(y + x, (H,), w[P + "output.LayerNorm.weight"], w[P + "output.LayerNorm.bias"], eps)
        i += 1
    return x


def text_features(w, input_ids, attention_mask, heads: int = 12, masks: Optional[Dict] = None):
    return E.masked_meanpool_l2(bert_last_hidden_state(w, input_ids, attention_mask, heads, masks=masks), attention_mask)


def vit_pooled(w, pixels, heads: int = 12, eps: float = 1e-5, masks: Optional[Dict] = None):
    V = "vision_model."
    pw = w[V + "embeddings.patch_embedding.weight"]
    H, patch = pw.shape[0], pw.shape[-1]
    N = pixels.shape[0]
    x = F.conv2d(pixels.to(pw.dtype), pw, bias=None, stride=patch).flatten(2).transpose(1, 2)
    cls = w[V + "embeddings.class_embedding"].expand(N, 1, H)
    x = torch.cat([cls, x], dim=1) + w[V + "embeddings.position_embedding.weight"][None]
    x = F.layer_norm(x, (H,), w[V + "pre_layrnorm.weight"], w[V + "pre_layrnorm.bias"], eps)
    i = 0
    while V + f"encoder.layers.{i}.self_attn.q_proj.weight" in w:
        P = V + f"encoder.layers.{i}."
        h = F.layer_norm(x, (H,), w[P + "layer_norm1.weight"], w[P + "layer_norm1.bias"], eps)
        ctx = _mha(h, w[P + "self_attn.q_proj.weight"], w[P + "self_attn.q_proj.bias"],
                   w[P + "self_attn.k_proj.weight"], w[P + "self_attn.k_proj.bias"],
                   w[P + "self_attn.v_proj.weight"], w[P + "self_attn.v_proj.bias"], heads, None,
                   None if masks is None else masks.get(("attn", i)))
        x = x + F.linear(ctx, w[P + "self_attn.out_proj.weight"], w[P + "self_attn.out_proj.bias"])
        h = F.layer_norm(x, (H,), w[P + "layer_norm2.weight"], w[P + "layer_norm2.bias"], eps)
        h = F.linear(h, w[P + "mlp.fc1.weight"], w[P + "mlp.fc1.bias"])
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, w[P + "mlp.fc2.weight"], w[P + "mlp.fc2.bias"])
        i += 1
    return F.layer_norm(x[:, 0], (H,), w[V + "post_layernorm.weight"], w[V + "post_layernorm.bias"], eps)


def visual_features(w, frames, heads: int = 12, masks: Optional[Dict] = None):
    if frames.dim() == 4:
        frames = frames[:, None]
    B, Fr = frames.shape[:2]
    pooled = vit_pooled(w, frames.reshape(B * Fr, *frames.shape[2:]), heads, masks=masks)
    e = F.linear(pooled, w["visual_projection.weight"])
    e = e / (e.norm(dim=-1, keepdim=True) + 1e-9)
    e = e.view(B, Fr, -1)
    if Fr == 1:
        return e[:, 0]
    return E.field_mean_l2(e)


# --------------------------------------------------------------------------
def _grads(fn, w, seed: int, dtype):
    wl = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in w.items()}
    feat = fn(wl)
    g = torch.Generator().manual_seed(seed)
    (feat * torch.randn(feat.shape, generator=g).to(dtype)).sum().backward()        # oracle.encoders_ref.probe_loss
    return feat.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in wl.items()}


def text_feature_grads(w, input_ids, attention_mask, seed: int, heads: int = 12, masks: Optional[Dict] = None, dtype=torch.float64):
    """(features, {name: d probe_loss / d w[name]}) with the masks multiplied in, computed in `dtype`."""
    return _grads(lambda wl: text_features(wl, input_ids, attention_mask, heads, masks), w, seed, dtype)


def visual_feature_grads(w, frames, seed: int, heads: int = 12, masks: Optional[Dict] = None, dtype=torch.float64):
    return _grads(lambda wl: visual_features(wl, frames.to(dtype), heads, masks), w, seed, dtype)
