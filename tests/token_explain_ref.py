"""Autograd yardstick of the token / image-patch attributions (tests only): explain.input_attribution and the encoders'
data-gradient passes (encoder_train.TextBackprop / VisualBackprop.input_grad).

Everything is torch.autograd over oracle/encoders_ref.py and oracle.tier_a.forward_batch (the head yardstick of
tests/explain_ref.py), eval mode.  The text encoder and the head run in the dtype asked for (float64 by default); the visual
encoder runs in float32, because the oracle's vit_pooled casts its pixels to float32 (its error, ~1e-6, is four orders below the
bf16 bounds these references are used with).

Per-position embedding gradients without touching the oracle: the word table is replaced by its gathered rows (B L, H) and the ids
by arange(B L), so `table[ids]` is the same tensor and d / d table is the gradient at each position's raw embedding sum
s = word + position + type (ds / d table = I).  Pixel gradients: frames.requires_grad_().

Baselines as the product states them: text = position + type + word[pad_id], so s - base = table - word[pad_id]; vision = zero.
temporal_features are DATA (no gradient through align, held along an integration path)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from oracle import encoders_ref as E
from oracle import tier_a as O

WORD = "embeddings.word_embeddings.weight"


def rel_bound(layers: int) -> float:
    """tests/test_gpu_encoder_train.py: 2.5 x 2^-9 sqrt(4 n) -- 1.4e-2 at 2 layers (that file rounds it up to 1.6e-2), 3.4e-2 at 12."""
    return 2.5 * 2.0 ** -9 * (4.0 * layers) ** 0.5


def gathered(w: Dict[str, torch.Tensor], ids: torch.Tensor, dtype=torch.float64):
    """(weights with the word table replaced by its gathered rows, the matching ids = arange(B L) as (B, L))."""
    wl = {k: v.to(dtype) for k, v in w.items()}
    wl[WORD] = wl[WORD][ids.reshape(-1)].clone()
    return wl, torch.arange(ids.numel()).view_as(ids)


def text_input_grad(w, ids, mask, dfeat: torch.Tensor, dtype=torch.float64):
    """(features (B, H), d sum(features * dfeat) / d s (B L, H))."""
    wl, pos_ids = gathered(w, ids, dtype)
    wl[WORD].requires_grad_(True)
    feat = E.text_features(wl, pos_ids, mask)
    (g,) = torch.autograd.grad((feat * dfeat.to(dtype)).sum(), wl[WORD])
    return feat.detach(), g


def visual_input_grad(w, frames: torch.Tensor, dfeat: torch.Tensor):
    """(features (B, proj), d sum(features * dfeat) / d frames), float32."""
    fr = frames.float().clone().requires_grad_(True)
    feat = E.visual_features({k: v.float() for k, v in w.items()}, fr)
    (g,) = torch.autograd.grad((feat * dfeat.float()).sum(), fr)
    return feat.detach(), g


def patch_sums(pixels: torch.Tensor, patch: int) -> torch.Tensor:
    """(B, F, 3, S, S) -> (B, F, (S / patch)^2), patches in (row, column) order as the ViT's tokens."""
    B, Fr, Cc, S, _ = pixels.shape
    G = S // patch
    return pixels.reshape(B, Fr, Cc, G, patch, G, patch).sum(dim=(2, 4, 6)).reshape(B, Fr, G * G)


def input_attribution(fus, clf, wt, wv, batch: Dict[str, torch.Tensor], class_idx: int = 1, method: str = "grad_x_input", steps: int = 16,
                      pad_id: int = 0, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The product's explain.input_attribution: tokens, token_grad_norm, patches, pixels, logits (and delta), plus the
    Cauchy-Schwarz scales the comparisons are measured in: token_scale (B,) = sqrt(sum_l ||g_l||^2 ||s_l - base_l||^2) and
    patch_scale (B,) = sqrt(sum_patches ||g_patch||^2 ||x_patch||^2).  fus / clf: parameter dicts in `dtype`."""
    ids, mask, frames = batch["input_ids"], batch["attention_mask"].long(), batch["frames"].float()
    if frames.dim() == 4:
        frames = frames[:, None]
    B, Lq = ids.shape
    wl, pos_ids = gathered(wt, ids, dtype)
    wvf = {k: v.float() for k, v in wv.items()}
    table = wl[WORD]
    base = wt[WORD][pad_id].to(dtype)[None].expand_as(table)
    patch = wv["vision_model.embeddings.patch_embedding.weight"].shape[-1]
    rest = {k: v for k, v in batch.items() if k not in ("input_ids", "attention_mask", "frames")}
    rest.setdefault("label", torch.zeros(B, dtype=torch.int64))      # (forward_batch passes it through)

    def logits_at(tab: torch.Tensor, fr: torch.Tensor) -> torch.Tensor:
        b = dict(rest)
        b["text_features"] = E.text_features({**wl, WORD: tab}, pos_ids, mask)
        b["visual_features"] = E.visual_features(wvf, fr).to(dtype)
        return O.forward_batch(fus, clf, b, train=False)["logits"]

    def grads_at(alpha: Optional[float]):
        tab = (table if alpha is None else base + alpha * (table - base)).detach().requires_grad_(True)
        fr = (frames if alpha is None else alpha * frames).detach().requires_grad_(True)
        lg = logits_at(tab, fr)
        gt, gf = torch.autograd.grad(lg[:, class_idx].sum(), [tab, fr])
        return gt, gf.to(dtype), lg.detach()

    out = {}
    if method == "grad_x_input":
        gt, gf, out["logits"] = grads_at(None)
    elif method == "integrated_gradients":
        out["logits"] = grads_at(None)[2]
        gt, gf = torch.zeros_like(table), torch.zeros_like(frames, dtype=dtype)
        for k in range(steps):
            a, b, _ = grads_at((k + 0.5) / steps)
            gt += a
            gf += b
        gt /= steps
        gf /= steps
        with torch.no_grad():
            out["delta"] = (logits_at(table, frames) - logits_at(base, torch.zeros_like(frames)))[:, class_idx]
    else:
        raise ValueError(method)
    m = mask.to(dtype)
    d = table - base
    out["tokens"] = ((gt * d).sum(-1).view(B, Lq) * m).detach()
    out["token_grad_norm"] = (gt.norm(dim=-1).view(B, Lq) * m).detach()
    out["pixels"] = (gf * frames.to(dtype)).detach()
    out["patches"] = patch_sums(out["pixels"], patch)
    out["token_scale"] = ((gt.norm(dim=-1) * d.norm(dim=-1)).view(B, Lq) * m).norm(dim=1).detach()
    out["patch_scale"] = (patch_sums(gf * gf, patch).sqrt() * patch_sums(frames.to(dtype) ** 2, patch).sqrt()).flatten(1).norm(dim=1).detach()
    return out
