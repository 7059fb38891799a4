"""Autograd restatement of the classifier's explanation helpers and of the per-modality attribution (tests only).

  feature_importance   src/models/fusion/deep_truth_classifier.py:189-211, as its docstring states it for both `use_aux` settings
  smooth_grad          the smooth-grad branch of explain_shap, :251-272 (the branch the reference takes: `shap` is not installed)
  modality_attribution the same gradient x input carried through forward_batch to the six inputs of the trainer

Every function is torch.autograd.grad over oracle.tier_a.classifier_forward / forward_batch, eval mode, in the dtype of the
parameters it is given: float32 reproduces the reference bit for bit (tests/golden/make_golden_explain.py checks that before it
writes tests/golden/explain.npz), float64 is the yardstick the HIP kernels are measured against.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from oracle import tier_a as O

STEPS = 16        # N of the reference's loop (:261)
INPUTS = ("text_features", "audio_features", "visual_features", "temporal_features", "gnn_feat", "aux")


def _x(clf: Dict[str, torch.Tensor], fused: torch.Tensor, aux: Optional[torch.Tensor]) -> torch.Tensor:
    """cat[fused, aux] in the parameters' dtype; a classifier built with `use_aux: false` ignores aux (:142-146)."""
    dt = clf["pre.0.weight"].dtype
    aux_w = O.clf_geometry(clf)[2]
    x = fused.to(dt)
    if aux_w > 0:
        x = torch.cat([x, aux.to(dt)], dim=-1)
    return x


def _forward(clf, x):
    H = clf["pre.3.weight"].shape[1]
    return O.classifier_forward(clf, x[:, :H], x[:, H:] if x.shape[1] > H else None, train=False)


def feature_importance(clf, fused, aux=None, class_idx: int = 1):
    """(|d sum_b logits[b, class_idx] / dx * x| (B, F+A), its mean over the rows (F+A,))."""
    x = _x(clf, fused, aux).detach().requires_grad_(True)
    (g,) = torch.autograd.grad(_forward(clf, x)["logits"][:, class_idx].sum(), x)
    imp = (g * x).abs().detach()
    return imp, imp.mean(dim=0)


def smooth_grad(clf, fused, aux, noise: torch.Tensor, max_samples: int = 256, walk: bool = True,
                rows: Optional[Sequence[int]] = None) -> torch.Tensor:
    """values (B', F+A), B' = min(B, max_samples): mean over 16 points of |d sum_b probs[b, 1] / dX|.  `noise`: the (16, B', F+A)
    draws of the reference's loop.  walk=True: the reference's points, X_i = X_{i-1} + noise_{i-1} * sigma (the 16th draw is
    unused).  walk=False: independent perturbations X_0 + noise_{i-1} * sigma of the same draws -- NOT what the reference does; the
    tests use it to show that they can tell the two apart.  `rows`: evaluate these rows only (sigma still comes from all B' rows)."""
    X = _x(clf, fused, aux)[:max_samples].detach()
    sigma = 0.1 * X.std(dim=0, keepdim=True).clamp_min(1e-6)
    noise = noise.to(X.dtype)
    if rows is not None:
        idx = torch.as_tensor(list(rows), dtype=torch.int64)
        X, noise = X[idx], noise[:, idx]
    X0, total = X, torch.zeros_like(X)
    for i in range(STEPS):
        x = X.detach().requires_grad_(True)
        (g,) = torch.autograd.grad(_forward(clf, x)["probs"][:, 1].sum(), x)
        total += g.abs()
        X = (X + noise[i] * sigma) if walk else (X0 + noise[i] * sigma)
    return total / STEPS


def modality_attribution(fus, clf, batch: Dict[str, torch.Tensor], class_idx: int = 1) -> Dict[str, torch.Tensor]:
    """{name: |d sum_b logits[b, class_idx] / d input * input|} for the inputs that reach the logits (no gnn_feat without gnn_proj, no
    aux without aux columns in pre.0).  The evidence scalars carry no gradient (oracle.tier_a.fusion_forward, as the reference)."""
    dt = clf["pre.0.weight"].dtype
    names = [n for n in INPUTS if not (n == "gnn_feat" and "gnn_proj.weight" not in fus) and not (n == "aux" and O.clf_geometry(clf)[2] == 0)]
    b = {k: (v.to(dt).detach().requires_grad_(k in names) if v.dtype.is_floating_point else v) for k, v in batch.items()}
    out = O.forward_batch(fus, clf, b, train=False)
    grads = torch.autograd.grad(out["logits"][:, class_idx].sum(), [b[n] for n in names])
    return {n: (g * b[n]).abs().detach() for n, g in zip(names, grads)}
