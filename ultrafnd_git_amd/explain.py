"""Per-modality attribution: the classifier's gradient x input (deep_truth_classifier.py:189-211) carried through BOTH modules
of the head to the six inputs the trainer feeds (forensic_trainer.py:238-271).

    ufnd_fusion_forward -> ufnd_classifier_input_grad (d_fused, d_aux; no parameter gradient)
        -> ufnd_fusion_backward_phase(UFND_BWD_ALL | UFND_BWD_NO_LINEAR_GRADS) -> ufnd_fusion_input_grads -> ufnd_attribution_reduce

Eval mode (no dropout) whatever the modules' mode, which is left as found.  The evidence scalars carry no gradient, as in the
reference (`no_grad`, cross_modal_transformer.py:153-164).  The fusion backward is a backward like any other: it OVERWRITES the
fusion's small non-Linear gradients (the evidence gates') in the gradient arena and the activations in the fusion's grad
workspace of this batch size -- a forward of that size still waiting for its `backward()` raises there instead of reading them.
No Linear weight gradient and nothing of the classifier's is written; parameters are untouched.
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
    B, H, W, ld = xs["text_features"].shape[0], clf.hidden, clf.hidden + clf.eff_aux, clf.hidden + 4
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
    clf._input_grad(clf._explain_ws(B), fused.data_ptr(), H, xs.get("aux"), B, False, L.TARGET_LOGIT, class_idx, gx)
    fusion._arena.ensure_grad()
    L.check(lib.ufnd_fusion_backward_phase(C.byref(fd), C.byref(fusion.param_table()), C.byref(fusion.grad_table()), *ins, gnn, B, 0,
                                           fws.data_ptr(), gx.data_ptr(), ld, None, state, s, None, 1, L.BWD_ALL | L.BWD_NO_LINEAR_GRADS),
            "ufnd_fusion_backward_phase")
    grads = {n: torch.empty_like(xs[n]) for n in names if n != "aux"}
    L.check(lib.ufnd_fusion_input_grads(C.byref(fd), C.byref(fusion.param_table()), fws.data_ptr(), B, *[L.ptr(grads.get(n)) for n in ORDER[:5]],
                                        state, s), "ufnd_fusion_input_grads")
    out = {}
    for n in names:
        g_ptr, ldg = (gx.data_ptr() + 4 * H, ld) if n == "aux" else (grads[n].data_ptr(), widths[n])
        out[n] = torch.empty(B, widths[n], dtype=f32, device=dev)
        L.check(lib.ufnd_attribution_reduce(L.ATTR_GRAD_X_INPUT, g_ptr, ldg, xs[n].data_ptr(), widths[n], B, widths[n], 1, 0, 0,
                                            out[n].data_ptr(), widths[n], None, None, s), "ufnd_attribution_reduce")
    return {"inputs": out, "modality": torch.stack([out[n].sum(dim=1) for n in names], dim=1), "order": tuple(names)}
