"""Per-modality attribution: the classifier's gradient x input (deep_truth_classifier.py:189-211) carried through BOTH modules
of the head to the six inputs the trainer feeds (forensic_trainer.py:238-271).

    ufnd_fusion_forward -> ufnd_classifier_input_grad (d_fused, d_aux; no parameter gradient)
        -> ufnd_fusion_backward_phase(UFND_BWD_ALL | UFND_BWD_NO_LINEAR_GRADS) -> ufnd_fusion_input_grads -> ufnd_attribution_reduce

Eval mode (no dropout) whatever the modules' mode, which is left as found.  The evidence scalars carry no gradient, as in the
reference (`no_grad`, cross_modal_transformer.py:153-164).  The fusion backward is a backward like any other: it OVERWRITES the
fusion's small non-Linear gradients (the evidence gates') in the gradient arena and the activations in the fusion's grad
workspace of this batch size -- a forward of that size still waiting for its `backward()` raises there instead of reading them.
No Linear weight gradient and nothing of the classifier's is written; parameters are untouched.

Token and image-patch attribution (`input_attribution`): the same head gradients carried on through BOTH encoders.

    TextBackprop / VisualBackprop.forward_saved -> the head as above (raw input gradients) -> .input_grad / .patch_grad
    (encoder_train.py: the data-gradient chain only) -> ufnd_token_attribution, ufnd_vit_unpatchify_attribution

`integrated_gradients` walks the straight path from the baselines (ufnd_path_points) in chunks of whole steps and averages
the gradients in step order (ufnd_attribution_reduce, UFND_ATTR_PATH_MEAN).  The encoders may be frozen or bound to a
trainer's arena; neither their parameters nor any encoder gradient is written.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib as L

ORDER = ("text_features", "audio_features", "visual_features", "temporal_features", "gnn_feat", "aux")


def modality_attribution(fusion, clf, feats: Dict[str, torch.Tensor], aux: Optional[torch.Tensor], class_idx: int = 1) -> Dict[str, object]:
    """{"inputs": {name: |d sum_b logits[b, class_idx] / d x * x| (B, width)}, "modality": (B, len(order)) row sums,
    "order": the names}.  `gnn_feat` is absent with fusion.yaml's `use_gnn: false`, `aux` with classifier.yaml's
    `use_aux: false` (neither reaches the logits then)."""
    if class_idx not in (0, 1):
        raise ValueError(f"modality_attribution: class_idx={class_idx}: the head has two classes (0, 1)")
    if fusion.hidden != clf.hidden:
        raise ValueError(f"modality_attribution: fusion hidden_dim {fusion.hidden} != classifier hidden_dim {clf.hidden}")
    names = [n for n in ORDER[:4]] + (["gnn_feat"] if fusion.use_gnn else []) + (["aux"] if clf.eff_aux else [])
    widths = {"text_features": 768, "audio_features": 128, "visual_features": 512, "temporal_features": 256,
              "gnn_feat": fusion.gnn_dim, "aux": clf.eff_aux}
    xs = {}
    for n in names:
        x = aux if n == "aux" else feats.get(n)
        if x is None:
            raise RuntimeError(f"modality_attribution: {n} is required")
        if x.dim() != 2 or x.shape[1] != widths[n] or x.shape[0] != feats["text_features"].shape[0]:
            raise RuntimeError(f"modality_attribution: {n}: expected (B,{widths[n]}), got {tuple(x.shape)}")
        xs[n] = x
    dev = fusion._arena.device
    if dev.type != "cuda" or clf._arena.device.type != "cuda":
        raise L.UltrafndHipError("modality_attribution runs on a HIP device only: move both modules to 'cuda' (there is no CPU fallback)")
    L.require_hip(*xs.values(), fusion._arena.data, clf._arena.data)
    xs = {n: L.f32c(x) for n, x in xs.items()}
    grads, gx, _ = _head_input_grads(fusion, clf, xs, class_idx)
    B, H, ld = xs["text_features"].shape[0], clf.hidden, clf.hidden + 4
    lib, s, f32 = L.lib(), L.stream_ptr(dev), torch.float32
    out = {}
    for n in names:
        g_ptr, ldg = (gx.data_ptr() + 4 * H, ld) if n == "aux" else (grads[n].data_ptr(), widths[n])
        out[n] = torch.empty(B, widths[n], dtype=f32, device=dev)
        L.check(lib.ufnd_attribution_reduce(L.ATTR_GRAD_X_INPUT, g_ptr, ldg, xs[n].data_ptr(), widths[n], B, widths[n], 1, 0, 0,
                                            out[n].data_ptr(), widths[n], None, None, s), "ufnd_attribution_reduce")
    return {"inputs": out, "modality": torch.stack([out[n].sum(dim=1) for n in names], dim=1), "order": tuple(names)}


def _head_input_grads(fusion, clf, xs: Dict[str, torch.Tensor], class_idx: int, inputs: bool = True):
    """Both modules' eval-mode forward on contiguous fp32 device inputs `xs` (the names of ORDER that reach the logits) and the raw
    gradients of sum_b logits[b, class_idx]: ({name: (B, width)} for the fusion's inputs, gx (B, hidden + 4) = [d_fused | d_aux |
    pad], logits (B, 2)).  inputs=False stops after the classifier (logits only: no fusion backward, the dict is empty)."""
    dev = fusion._arena.device
    B, H, ld = xs["text_features"].shape[0], clf.hidden, clf.hidden + 4
    lib, s, f32 = L.lib(), L.stream_ptr(dev), torch.float32
    fd, state = fusion.dims(), fusion.rng().ptr
    fws = fusion.workspace(B, True)
    fusion._gen[B] = fusion._gen.get(B, 0) + 1      # the saved activations of a pending backward of this size are gone
    gnn = xs["gnn_feat"].data_ptr() if fusion.use_gnn else None
    ins = [xs[n].data_ptr() for n in ORDER[:4]]
    fused = torch.empty(B, H, dtype=f32, device=dev)
    forensic = torch.empty(3, B, dtype=f32, device=dev)
    L.check(lib.ufnd_fusion_forward(C.byref(fd), C.byref(fusion.param_table()), *ins, gnn, B, 0, fws.data_ptr(), fused.data_ptr(), H, None,
                                    forensic.data_ptr(), state, s), "ufnd_fusion_forward")
    gx = torch.empty(B, ld, dtype=f32, device=dev)      # [d_fused | d_aux | pad]
    logits, _ = clf._input_grad(clf._explain_ws(B), fused.data_ptr(), H, xs.get("aux"), B, False, L.TARGET_LOGIT, class_idx, gx)
    if not inputs:
        return {}, gx, logits
    fusion._arena.ensure_grad()
    L.check(lib.ufnd_fusion_backward_phase(C.byref(fd), C.byref(fusion.param_table()), C.byref(fusion.grad_table()), *ins, gnn, B, 0,
                                           fws.data_ptr(), gx.data_ptr(), ld, None, state, s, None, 1, L.BWD_ALL | L.BWD_NO_LINEAR_GRADS),
            "ufnd_fusion_backward_phase")
    grads = {n: torch.empty_like(xs[n]) for n in xs if n != "aux"}
    L.check(lib.ufnd_fusion_input_grads(C.byref(fd), C.byref(fusion.param_table()), fws.data_ptr(), B, *[L.ptr(grads.get(n)) for n in ORDER[:5]],
                                        state, s), "ufnd_fusion_input_grads")
    return grads, gx, logits


# ------------------------------------------------------------------------------------------------ tokens and image patches
METHODS = ("grad_x_input", "integrated_gradients")


def _backprop(enc, cls):
    """`enc`: an encoder (frozen: an unbound backprop object is kept on it, its operand copies follow `weights_version`) or the
    TextBackprop / VisualBackprop a trainer has bound to its arena (its masters and operand copies are used as they stand)."""
    if isinstance(enc, cls):
        return enc
    bp = getattr(enc, "_input_bp", None)
    if bp is None:
        bp = enc._input_bp = cls(enc)
    return bp


def _path_points(x: torch.Tensor, base: Optional[torch.Tensor], alphas, rows: int, width: int) -> torch.Tensor:
    out = torch.empty(len(alphas) * rows, width, dtype=torch.float32, device=x.device)
    arr = (C.c_float * len(alphas))(*alphas)
    L.check(L.lib().ufnd_path_points(x.data_ptr(), L.ptr(base), arr, len(alphas), rows, width, out.data_ptr(), L.stream_ptr(x.device)),
            "ufnd_path_points")
    return out


def input_attribution(fusion, clf, text_encoder, visual_encoder, batch: Dict[str, torch.Tensor], class_idx: int = 1,
                      method: str = "grad_x_input", steps: int = 16, pad_id: int = 0, rows_per_pass: int = 16384, *,
                      temporal_net=None) -> Dict[str, torch.Tensor]:
    """Which tokens and which image regions a logit is owed to: the gradient of sum_b logits[b, class_idx] carried through the head
    and both encoders to the text encoder's raw embedding sums s (word + position + type, before their LayerNorm) and to the pixels.

    `batch`: input_ids (B, L), attention_mask (B, L), frames (B, F, 3, S, S) or (B, 3, S, S), audio_features, and -- where the
    configuration uses them -- gnn_feat, aux; temporal_features, or `temporal_net=` (TemporalSyncNet: its deterministic align of the
    encoders' features, as the trainer's evaluation does).  temporal is DATA: computed once at the input, held along the path, and
    no gradient flows through align (as in training).  Eval mode throughout: no dropout in the head or in the encoders.
    `text_encoder` / `visual_encoder`: the encoders (frozen), or a trainer's bound TextBackprop / VisualBackprop.

    Baselines: text = position + type + word[pad_id] per position; vision = a zero frame.
      grad_x_input          g (x - base), g the gradient at the input
      integrated_gradients  the same with g averaged over the midpoints alpha_k = (k + 1/2) / steps of the straight path from the
                            baselines to the input (text and frames move together), evaluated in chunks of whole steps of at most
                            rows_per_pass token rows, added in step order.  Also "delta" (B,) = logit(input) - logit(baselines): the
                            sum of all token and pixel scores of a sample converges to it as steps grow.
    Returns device tensors: tokens (B, L) = sum_h g (s - base) (0 on masked tokens), token_grad_norm (B, L) = ||g||_2, patches
    (B, F, P) per-patch sums of pixels (B, F, 3, S, S) = g (x - base), logits (B, 2)."""
    from .encoder_train import TextBackprop, VisualBackprop
    if class_idx not in (0, 1):
        raise ValueError(f"input_attribution: class_idx={class_idx}: the head has two classes (0, 1)")
    if method not in METHODS:
        raise ValueError(f"input_attribution: method={method!r}: one of {METHODS}")
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"input_attribution: steps={steps}: at least 1")
    if fusion.hidden != clf.hidden:
        raise ValueError(f"input_attribution: fusion hidden_dim {fusion.hidden} != classifier hidden_dim {clf.hidden}")
    tbp, vbp = _backprop(text_encoder, TextBackprop), _backprop(visual_encoder, VisualBackprop)
    te, ve = tbp.enc, vbp.enc
    dev = fusion._arena.device
    if any(d.type != "cuda" for d in (dev, clf._arena.device, te.device, ve.device)):
        raise L.UltrafndHipError("input_attribution runs on a HIP device only: move the head and both encoders to 'cuda' (there is no CPU fallback)")
    if not 0 <= int(pad_id) < te.vocab:
        raise ValueError(f"input_attribution: pad_id={pad_id} outside the vocabulary [0, {te.vocab})")
    for n in ("input_ids", "attention_mask", "frames", "audio_features"):
        if batch.get(n) is None:
            raise RuntimeError(f"input_attribution: batch[{n!r}] is required")
    ids, mask = batch["input_ids"].to(dev), batch["attention_mask"].to(dev, torch.int32).contiguous()
    frames = L.f32c(vbp._frames5(batch["frames"]).to(dev))
    B, Lq = ids.shape
    Fr, S, p, P, H = frames.shape[1], ve.image, ve.patch, ve.n_patches, te.hidden
    M, N, NP, K, FW = B * Lq, B * Fr, B * Fr * P, 3 * p * p, 3 * S * S
    if tuple(mask.shape) != (B, Lq) or frames.shape[0] != B:
        raise RuntimeError(f"input_attribution: attention_mask {tuple(mask.shape)} / frames {tuple(frames.shape)} do not match input_ids ({B},{Lq})")
    lib, s, f32 = L.lib(), L.stream_ptr(dev), torch.float32

    # the batch: encoder forwards (activations saved), temporal, the head's raw input gradients
    xs = {"text_features": tbp.forward_saved(ids, mask), "visual_features": vbp.forward_saved(frames)}
    sums = tbp.xsaved["s"]
    xs["audio_features"] = L.f32c(batch["audio_features"].to(dev))
    if batch.get("temporal_features") is not None:
        xs["temporal_features"] = L.f32c(batch["temporal_features"].to(dev))
    elif temporal_net is not None:
        xs["temporal_features"] = temporal_net.align_batch(xs["text_features"], xs["visual_features"], training=False)
    else:
        raise RuntimeError("input_attribution: batch['temporal_features'] or temporal_net= is required")
    for n, use in (("gnn_feat", fusion.use_gnn), ("aux", bool(clf.eff_aux))):
        if use:
            if batch.get(n) is None:
                raise RuntimeError(f"input_attribution: batch[{n!r}] is required")
            xs[n] = L.f32c(batch[n].to(dev))
    widths = {"audio_features": 128, "temporal_features": 256, "gnn_feat": fusion.gnn_dim, "aux": clf.eff_aux}
    for n, wd in widths.items():
        if n in xs and tuple(xs[n].shape) != (B, wd):
            raise RuntimeError(f"input_attribution: {n}: expected ({B},{wd}), got {tuple(xs[n].shape)}")
    grads, _, logits = _head_input_grads(fusion, clf, xs, class_idx)

    # baselines: the embedding sums of an all-pad_id row per position; a zero frame (base = NULL in the kernels)
    w = te._w
    base = torch.empty(M, H, dtype=f32, device=dev)
    pad = torch.full((B, Lq), int(pad_id), dtype=torch.int64, device=dev)
    L.check(lib.ufnd_bert_embed(pad.data_ptr(), w["embeddings.word_embeddings.weight"].data_ptr(), w["embeddings.position_embeddings.weight"].data_ptr(),
                                w["embeddings.token_type_embeddings.weight"].data_ptr(), None, None, None, base.data_ptr(), B, Lq, H, te.vocab, te.eps, s),
            "ufnd_bert_embed")

    out = {"logits": logits}
    if method == "grad_x_input":
        g_tok, g_patch = tbp.input_grad(grads["text_features"]), vbp.patch_grad(grads["visual_features"])
    else:
        alphas = [(k + 0.5) / steps for k in range(steps)]
        per = max(1, min(int(rows_per_pass) // M, L.MAX_ROWS // max(M, NP, 1), L.PATH_MAX_POINTS, steps))
        if per * max(M, NP) > L.MAX_ROWS:
            raise ValueError(f"input_attribution: one step is {max(M, NP)} rows: a pass takes at most {L.MAX_ROWS}")
        g_tok, g_patch = torch.empty(M, H, dtype=f32, device=dev), torch.empty(NP, K, dtype=f32, device=dev)
        rest = {n: x for n, x in xs.items() if n not in ("text_features", "visual_features")}
        for k0 in range(0, steps, per):
            c = min(per, steps - k0)
            s_pts = _path_points(sums, base, alphas[k0:k0 + c], M, H)
            f_pts = _path_points(frames, None, alphas[k0:k0 + c], N, FW).view(c * B, Fr, 3, S, S)
            pts = {"text_features": tbp.forward_saved(None, mask.repeat(c, 1), sums=s_pts), "visual_features": vbp.forward_saved(f_pts)}
            pts.update({n: x.repeat(c, 1) for n, x in rest.items()})
            gc, _, _ = _head_input_grads(fusion, clf, {n: pts[n] for n in xs}, class_idx)
            last = k0 + c == steps
            for G, acc, rows, wd in ((tbp.input_grad(gc["text_features"]), g_tok, M, H), (vbp.patch_grad(gc["visual_features"]), g_patch, NP, K)):
                L.check(lib.ufnd_attribution_reduce(L.ATTR_PATH_MEAN, G.data_ptr(), wd, None, 0, rows, wd, c, int(k0 > 0), steps if last else 0,
                                                    acc.data_ptr(), wd, None, None, s), "ufnd_attribution_reduce")
        # completeness: logit(input) - logit(baselines), both ends in ONE forward of 2 B samples (temporal and the rest held)
        ends = {"text_features": tbp.forward_saved(None, mask.repeat(2, 1), sums=torch.cat([sums, base], 0)),
                "visual_features": vbp.forward_saved(torch.cat([frames, torch.zeros_like(frames)], 0))}
        ends.update({n: x.repeat(2, 1) for n, x in rest.items()})
        _, _, lg = _head_input_grads(fusion, clf, {n: ends[n] for n in xs}, class_idx, inputs=False)
        out["delta"] = lg[:B, class_idx] - lg[B:, class_idx]
    tokens, norm = torch.empty(B, Lq, dtype=f32, device=dev), torch.empty(B, Lq, dtype=f32, device=dev)
    L.check(lib.ufnd_token_attribution(g_tok.data_ptr(), H, sums.data_ptr(), H, base.data_ptr(), H, mask.data_ptr(), M, H, tokens.data_ptr(),
                                       norm.data_ptr(), s), "ufnd_token_attribution")
    pixels, patches = torch.empty_like(frames), torch.empty(B, Fr, P, dtype=f32, device=dev)
    L.check(lib.ufnd_vit_unpatchify_attribution(g_patch.data_ptr(), frames.data_ptr(), None, None, pixels.data_ptr(), patches.data_ptr(), N, S, p, s),
            "ufnd_vit_unpatchify_attribution")
    out.update({"tokens": tokens, "token_grad_norm": norm, "patches": patches, "pixels": pixels})
    return out
