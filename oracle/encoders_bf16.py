"""TEST INFRASTRUCTURE (see oracle/__init__.py) -- the text encoder's gradients with the HIP backward's bf16 roundings emulated.

oracle/encoders_ref.py gives the fp32 autograd of the encoder restatement; the trainable-encoder path
(ultrafnd_git_amd/encoder_train.py) rounds to bf16 at fixed points of its forward and backward and accumulates in fp32.  This
module recomputes `text_feature_grads` with torch.autograd.Function wrappers that round exactly there, so that a test can tell
an error every bf16 implementation pays from an error of one kernel, and an ablation can tell which rounding carries it.

Rounding points (the set of active ones is an argument; ALL is the kernel emulation):

  forward
    "x"      LayerNorm outputs written bf16 as GEMM inputs (embeddings, attention.output, output LayerNorm)
             -- encoder_train.py:340,347,352 (the fp32 copies that feed the residual sums stay fp32)
    "w"      every Linear's weight as bf16 W (forward, weight-gradient shape) and W^T (data gradient), the same values
             -- encoder_train.py:120-160 (refresh_operands)
    "qkv"    the fused q|k|v rows written bf16 -- encoder_train.py:344
    "p_fwd"  the attention forward's P rounded to bf16 before P V -- attention.hip:141-169 (the kernel rounds the unnormalised
             exp2(s - m) and divides by the fp32 row sum afterwards; here the normalised P is rounded: the same relative rounding)
    "ctx"    the attention output written bf16 -- encoder_train.py:345, attention.hip:187
    "pre"    FFN1's pre-activations written bf16 (the GELU derivative of the backward is taken at them) -- encoder_train.py:348
    "act"    the GELU output written bf16 (FFN2's input) -- encoder_train.py:349
  The LayerNorm input sums (ctx W_o + b + x, h W_2 + b + x1) and the residual stream stay fp32 (encoder_train.py:346,350):
  they are not rounding points.
  backward
    "dy"     the LayerNorm backward's bf16 dx: the dy operand of output.dense and attention.output.dense (weight gradient, bias
             gradient and data gradient) -- encoder_train.py:376-378,382-384; the fp32 dx continues along the residual
    "dpre"   d loss / d pre, formed in fp32 in the data-gradient epilogue (x GELU'(pre)) and written bf16 -- encoder_train.py:378
    "dctx"   d loss / d ctx written bf16 (the attention backward's dO) -- encoder_train.py:384
    "delta"  delta_i = sum_d dO_id O_id from the bf16 ctx and dctx (attn_delta_kernel, attention_bwd.hip:6,56-74) instead of
             autograd's sum_j P_ij dP_ij (equal in exact arithmetic)
    "p_bwd"  P rounded to bf16 before dV = P^T dO -- attention_bwd.hip:176 (pf)
    "ds"     dS = P (dP - delta) / 8 rounded to bf16 before dQ = dS K and dK = dS^T Q -- attention_bwd.hip:176 (dsf)
    "dqkv"   the attention backward's output written bf16: the dy operand of the q/k/v Linear -- encoder_train.py:385-387

GEMM_OPERANDS are the roundings of the four Linears' operands (forward, weight gradient, data gradient): what any implementation
with bf16 GEMM operands and fp32 accumulation pays.  ATTENTION_INTERNAL are the roundings inside and around the attention kernels.
With no point active, every operation is the one encoders_ref.py performs, in the same order: the gradients are bit-identical to
encoders_ref.text_feature_grads (test).
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch
import torch.nn.functional as F

from . import encoders_ref as E

GEMM_OPERANDS = ("x", "w", "ctx", "act", "dy", "dpre", "dqkv")
ATTENTION_INTERNAL = ("qkv", "p_fwd", "dctx", "delta", "p_bwd", "ds")
ALL = GEMM_OPERANDS + ATTENTION_INTERNAL + ("pre",)


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


class _Round(torch.autograd.Function):
    """Identity with the value rounded to bf16 in forward (fwd) and / or the incoming gradient rounded in backward (bwd)."""

    @staticmethod
    def forward(ctx, x, fwd: bool, bwd: bool):
        ctx.bwd = bwd
        return _bf(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (_bf(g) if ctx.bwd else g), None, None


def _r(x: torch.Tensor, fwd: bool = False, bwd: bool = False) -> torch.Tensor:
    return _Round.apply(x, fwd, bwd) if (fwd or bwd) else x


class _AttnCore(torch.autograd.Function):
    """softmax(q k^T d^-1/2 + mask) v with the flash backward's formulation: delta from O and dO, P and dS rounded to bf16 before
    their products, as the flags say (q, k, v: (B, heads, L, d))."""

    @staticmethod
    def forward(ctx, q, k, v, add_mask, p_fwd: bool, ctx_bf16: bool, delta_o: bool, p_bwd: bool, ds_bf16: bool):
        scale = q.shape[-1] ** -0.5
        s = (q @ k.transpose(-1, -2)) * scale
        if add_mask is not None:
            s = s + add_mask
        p = torch.softmax(s, dim=-1)
        out = (_bf(p) if p_fwd else p) @ v
        ctx.save_for_backward(q, k, v, p, _bf(out) if ctx_bf16 else out)
        ctx.flags, ctx.scale = (delta_o, p_bwd, ds_bf16), scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, p, out = ctx.saved_tensors
        delta_o, p_bwd, ds_bf16 = ctx.flags
        dp = dout @ v.transpose(-1, -2)
        dv = (_bf(p) if p_bwd else p).transpose(-1, -2) @ dout
        delta = (dout * out).sum(-1, keepdim=True) if delta_o else (dp * p).sum(-1, keepdim=True)
        ds = p * (dp - delta) * ctx.scale
        if ds_bf16:
            ds = _bf(ds)
        return ds @ k, ds.transpose(-1, -2) @ q, dv, None, None, None, None, None, None


def _mha(x, wq, bq, wk, bk, wv, bv, heads: int, add_mask, on, lin):
    """encoders_ref._mha with the rounding points of the attention block (x: the bf16 LayerNorm output when "x" is active)."""
    B, L, H = x.shape
    d = H // heads
    q = lin(x, wq, bq, on("qkv"), on("dqkv")).view(B, L, heads, d).transpose(1, 2)
    k = lin(x, wk, bk, on("qkv"), on("dqkv")).view(B, L, heads, d).transpose(1, 2)
    v = lin(x, wv, bv, on("qkv"), on("dqkv")).view(B, L, heads, d).transpose(1, 2)
    if any(on(n) for n in ("p_fwd", "delta", "p_bwd", "ds")):
        o = _AttnCore.apply(q, k, v, add_mask, on("p_fwd"), on("ctx"), on("delta"), on("p_bwd"), on("ds"))
    else:                                   # encoders_ref._mha's own operations
        s = (q @ k.transpose(-1, -2)) * (d ** -0.5)
        if add_mask is not None:
            s = s + add_mask
        o = torch.softmax(s, dim=-1) @ v
    return _r(o.transpose(1, 2).reshape(B, L, H), on("ctx"), on("dctx"))


def bert_last_hidden_state(w: Dict[str, torch.Tensor], input_ids, attention_mask, points: Iterable[str] = ALL, heads: int = 12,
                           eps: float = 1e-12, collect: Optional[dict] = None) -> torch.Tensor:
    """encoders_ref.bert_last_hidden_state with the HIP training path's bf16 roundings at `points`."""
    pts = frozenset(points)
    unknown = pts - set(ALL)
    if unknown:
        raise ValueError(f"unknown rounding points {sorted(unknown)}; known: {ALL}")
    on = pts.__contains__

    def lin(x, wt, b, out_fwd, out_bwd):
        return _r(F.linear(x, _r(wt, on("w")), b), out_fwd, out_bwd)

    B, L = input_ids.shape
    H = w["embeddings.word_embeddings.weight"].shape[1]
    x = (w["embeddings.word_embeddings.weight"][input_ids]
         + w["embeddings.position_embeddings.weight"][:L][None]
         + w["embeddings.token_type_embeddings.weight"][0][None, None])
    x = F.layer_norm(x, (H,), w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], eps)
    add_mask = (1.0 - attention_mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    i = 0
    while f"encoder.layer.{i}.attention.self.query.weight" in w:
        P = f"encoder.layer.{i}."
        ctx = _mha(_r(x, on("x")), w[P + "attention.self.query.weight"], w[P + "attention.self.query.bias"],
                   w[P + "attention.self.key.weight"], w[P + "attention.self.key.bias"],
                   w[P + "attention.self.value.weight"], w[P + "attention.self.value.bias"], heads, add_mask, on, lin)
        y = lin(ctx, w[P + "attention.output.dense.weight"], w[P + "attention.output.dense.bias"], False, on("dy"))
        x = F.layer_norm(y + x, (H,), w[P + "attention.output.LayerNorm.weight"],
                         w[P + "attention.output.LayerNorm.bias"], eps)
        h = _r(F.gelu(lin(_r(x, on("x")), w[P + "intermediate.dense.weight"], w[P + "intermediate.dense.bias"], on("pre"), on("dpre"))),
               on("act"))
        y = lin(h, w[P + "output.dense.weight"], w[P + "output.dense.bias"], False, on("dy"))
        x = F.layer_norm(y + x, (H,), w[P + "output.LayerNorm.weight"], w[P + "output.LayerNorm.bias"], eps)
        i += 1
        if collect is not None:
            collect[i] = x
    return x


def text_feature_grads(w: Dict[str, torch.Tensor], input_ids, attention_mask, seed: int, points: Iterable[str] = ALL, heads: int = 12):
    """(features, {name: d probe_loss / d w[name]}) -- encoders_ref.text_feature_grads with the roundings at `points`."""
    wl = {k: v.detach().clone().requires_grad_(True) for k, v in w.items()}
    feat = E.masked_meanpool_l2(bert_last_hidden_state(wl, input_ids, attention_mask, points, heads), attention_mask)
    E.probe_loss(feat, seed).backward()
    return feat.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in wl.items()}
