"""DeepTruthClassifier -- MI355X-native mirror of the reference's NODE-ensemble classifier
(src/models/fusion/deep_truth_classifier.py:28-74,77-90,97-184).

Same constructor / YAML keys / `forward(fused, aux) -> {"logits","probs","temperature"}` /
`predict_proba` / `predict` / `state_dict` names and the same initialisation order.  The
arithmetic (pre-MLP, 6 soft oblivious trees, bypass, temperature softmax) runs in
libultrafnd_hip.so; there is no CPU path.

The interpretability helpers (:189-272) are here too: `feature_importance` (gradient x input at the logits) and
`explain_shap` (the reference's smooth-grad branch: mean |d probs[:, 1] / d x| over a 16-point random walk, evaluated as ONE
forward and one input-gradient backward over 16 B rows).  Both run `ufnd_classifier_input_grad`, which writes no parameter
gradient, on a workspace of their own.  `feature_importance` returns what the reference's docstring states for both
`use_aux` settings (the reference itself raises with the shipped `use_aux: true`); `explain_shap` never imports `shap`
(INTEGRATION.md section A).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .arena import ArenaModule, Group, rehome
from .config_utils import ConfigManager
from .state import StepStateBuffer


def _init_lin(m: nn.Linear):
    nn.init.xavier_uniform_(m.weight)
    if m.bias is not None:
        nn.init.zeros_(m.bias)


class _ObliviousTree(nn.Module):
    """Parameter container of one soft oblivious tree (deep_truth_classifier.py:36-52)."""

    def __init__(self, in_dim: int, num_classes: int = 2, depth: int = 4, tau: float = 10.0, dropout: float = 0.3):
        super().__init__()
        self.in_dim, self.depth, self.num_classes = in_dim, depth, num_classes
        self.tau = nn.Parameter(torch.tensor(float(tau)), requires_grad=False)
        self.gates = nn.ParameterList([nn.Parameter(torch.zeros(in_dim)) for _ in range(depth)])
        self.thresh = nn.ParameterList([nn.Parameter(torch.zeros(1)) for _ in range(depth)])
        self.num_leaves = 1 << depth
        self.leaf_logits = nn.Parameter(torch.zeros(self.num_leaves, num_classes))
        self.dropout = nn.Dropout(dropout)


class NODEEnsemble(nn.Module):
    def __init__(self, in_dim: int, num_classes: int = 2, num_trees: int = 6, depth: int = 4, tau: float = 10.0,
                 dropout: float = 0.3):
        super().__init__()
        self.trees = nn.ModuleList([_ObliviousTree(in_dim, num_classes, depth=depth, tau=tau, dropout=dropout)
                                    for _ in range(num_trees)])


class DeepTruthClassifier(ArenaModule):
    def __init__(self, config_path: str = "configs/model_configs/classifier.yaml"):
        super().__init__()
        cfg = ConfigManager().load_config(config_path)
        self.hidden = int(cfg.get("hidden_dim", 512))
        self.dropout = float(cfg.get("dropout", 0.3))
        self.num_classes = int(cfg.get("num_classes", 2))
        self.use_aux = bool(cfg.get("use_aux", True))
        self.aux_dim = int(cfg.get("aux_dim", 2))
        self.node_trees = int(cfg.get("node_trees", 6))
        self.node_depth = int(cfg.get("node_depth", 4))
        self.node_tau = float(cfg.get("node_tau", 10.0))
        self.node_dropout = 0.3   # hard-coded in the reference (deep_truth_classifier.py:132)
        self.temperature = nn.Parameter(torch.tensor(float(cfg.get("temperature", 1.0))), requires_grad=True)
        in_dim = int(cfg.get("input_dim", self.hidden))
        if in_dim != self.hidden:
            raise ValueError("input_dim must equal hidden_dim (the fusion head's output width)")
        # The reference's YAML takes any value here (deep_truth_classifier.py:106-117); the HIP kernels are built for the ranges
        # below (include/ultrafnd_hip.h, check_dims in csrc/tier_a.hip).  Refused at construction, naming the limit -- never at
        # the first forward on the device, and never silently.
        if self.num_classes != 2:
            raise ValueError(f"classifier.yaml: num_classes={self.num_classes}: the HIP path implements the reference's binary head (num_classes == 2)")
        if self.hidden not in (256, 512, 1024):
            raise ValueError(f"classifier.yaml: hidden_dim={self.hidden}: the HIP kernels support hidden_dim in {{256, 512, 1024}}")
        if not (1 <= self.node_depth <= 6 and 1 <= self.node_trees <= 16 and self.node_trees * self.node_depth <= 32):
            raise ValueError(f"classifier.yaml: node_trees={self.node_trees}, node_depth={self.node_depth}: the HIP kernels support "
                             "node_trees <= 16, node_depth <= 6 and node_trees x node_depth <= 32 (one lane per gate)")
        if self.use_aux and self.aux_dim not in (0, 2, 4):
            raise ValueError(f"classifier.yaml: aux_dim={self.aux_dim}: the HIP kernels support aux_dim in {{0, 2, 4}}")
        self.eff_aux = self.aux_dim if self.use_aux else 0
        self.pre = nn.Sequential(nn.Linear(in_dim + self.eff_aux, self.hidden), nn.GELU(), nn.Dropout(self.dropout),
                                 nn.Linear(self.hidden, self.hidden), nn.GELU(), nn.Dropout(self.dropout))
        for m in self.pre:
            if isinstance(m, nn.Linear):
                _init_lin(m)
        self.node = NODEEnsemble(self.hidden, self.num_classes, self.node_trees, self.node_depth, self.node_tau, self.node_dropout)
        self.bypass = nn.Linear(self.hidden, self.num_classes)
        _init_lin(self.bypass)
        self._ws: Dict[Tuple[int, bool], torch.Tensor] = {}
        self._xws: Optional[Tuple[int, torch.Tensor]] = None      # the explanations' own workspace (the latest row count only)
        self._ptab = self._gtab = None
        self._rng: Optional[StepStateBuffer] = None
        self._xrng: Optional[StepStateBuffer] = None              # ... and their own dropout key / counter (train-mode feature_importance)
        rehome([self], [""])

    # ------------------------------------------------------------------ arena layout
    def _arena_groups(self) -> Tuple[List[Group], List[Group]]:
        H, T, D = self.hidden, self.node_trees, self.node_depth
        pre = [("pre.0.weight", (H, H + self.eff_aux)), ("pre.0.bias", (H,)), ("pre.3.weight", (H, H)), ("pre.3.bias", (H,))]
        gates = [(f"node.trees.{t}.gates.{k}", (H,)) for t in range(T) for k in range(D)]
        thresh = [(f"node.trees.{t}.thresh.{k}", (1,)) for t in range(T) for k in range(D)]
        leaf = [(f"node.trees.{t}.leaf_logits", (1 << D, 2)) for t in range(T)]
        byp = [("bypass.weight", (2, H)), ("bypass.bias", (2,))]
        tau = [(f"node.trees.{t}.tau", ()) for t in range(T)]
        return [[p] for p in pre] + [gates, thresh, leaf] + [[b] for b in byp], [[("temperature", ())], tau]

    def _on_rehome(self) -> None:
        self._ptab = self._gtab = None
        self._ws.clear()
        self._xws = None
        self._rng = self._xrng = None

    def dims(self) -> L.Dims:
        d = L.Dims()
        d.hidden, d.text_dim, d.audio_dim, d.visual_dim, d.temporal_dim, d.gnn_dim = self.hidden, 768, 128, 512, 256, 128
        d.aux_dim, d.trees, d.depth, d.classes = self.eff_aux, self.node_trees, self.node_depth, 2
        d.fusion_dropout, d.clf_dropout, d.node_dropout = 0.1, self.dropout, self.node_dropout
        return d

    def _table(self, getter, with_nograd: bool) -> L.ClfParams:
        t = L.ClfParams()
        t.pre0_w, t.pre0_b = getter("pre.0.weight").data_ptr(), getter("pre.0.bias").data_ptr()
        t.pre3_w, t.pre3_b = getter("pre.3.weight").data_ptr(), getter("pre.3.bias").data_ptr()
        t.gates = getter("node.trees.0.gates.0").data_ptr()
        t.thresh = getter("node.trees.0.thresh.0").data_ptr()
        t.leaf = getter("node.trees.0.leaf_logits").data_ptr()
        t.bypass_w, t.bypass_b = getter("bypass.weight").data_ptr(), getter("bypass.bias").data_ptr()
        if with_nograd:
            t.tau = getter("node.trees.0.tau").data_ptr()
            t.temperature = getter("temperature").data_ptr()
        return t

    def param_table(self) -> L.ClfParams:
        if self._ptab is None:
            self._ptab = self._table(self.aview, True)
        return self._ptab

    def grad_table(self) -> L.ClfParams:
        if self._gtab is None:
            self._gtab = self._table(self.gview, False)
        return self._gtab

    def workspace(self, B: int, train: bool) -> torch.Tensor:
        key = (B, bool(train))
        if key not in self._ws:
            d = self.dims()
            n = L.lib().ufnd_clf_workspace_floats(C.byref(d), B)
            self._ws[key] = torch.empty(n, dtype=torch.float32, device=self._arena.device)
        return self._ws[key]

    def rng(self) -> StepStateBuffer:
        if self._rng is None:
            self._rng = StepStateBuffer(self._arena.device, seed=torch.initial_seed() + 0xC1F)
        return self._rng

    # ------------------------------------------------------------------ forward
    def forward(self, fused: torch.Tensor, aux: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        dev = self._arena.device
        if dev.type != "cuda":
            raise L.UltrafndHipError("DeepTruthClassifier runs on a HIP device only: call .to('cuda') "
                                     "(there is no CPU fallback)")
        fused = fused.to(dev, dtype=torch.float32)
        if self.use_aux and aux is None:
            raise RuntimeError(f"aux is required: pre.0 is built for {self.hidden}+{self.aux_dim} inputs "
                               "(the reference's Linear fails the same way, deep_truth_classifier.py:142-146,162)")
        aux = L.f32c(aux.to(dev)) if (self.use_aux and aux is not None) else None
        from .functional import ClassifierFunction
        needs_grad = torch.is_grad_enabled() and (fused.requires_grad or any(p.requires_grad for p in self.parameters()))
        logits, probs = ClassifierFunction.apply(self, self.training, needs_grad, fused, aux,
                                                 *[p for p in self.parameters() if p.requires_grad])
        t = torch.clamp(self.temperature, min=0.5, max=5.0)
        return {"logits": logits, "probs": probs, "temperature": t}

    @torch.no_grad()
    def predict_proba(self, fused: torch.Tensor, aux: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.forward(fused, aux)["probs"]

    @torch.no_grad()
    def predict(self, fused: torch.Tensor, aux: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.predict_proba(fused, aux).argmax(dim=-1)

    # ------------------------------------------------------------------ interpretability (deep_truth_classifier.py:189-272)
    SMOOTHGRAD_STEPS = 16      # N of the reference's smooth-grad loop (:261)

    def _explain_args(self, fused: torch.Tensor, aux: Optional[torch.Tensor], what: str):
        """The argument checks of both helpers, before anything touches a device: (fused, aux or None) as given."""
        if not isinstance(fused, torch.Tensor) or fused.dim() != 2 or fused.shape[1] != self.hidden:
            raise RuntimeError(f"{what}: fused: expected (B,{self.hidden}), got {tuple(getattr(fused, 'shape', ()))}")
        if fused.shape[0] < 1:
            raise ValueError(f"{what}: empty batch")
        if not self.use_aux:
            return fused, None      # a given aux is ignored, as in the reference (:142-146)
        if aux is None:
            raise RuntimeError(f"{what}: aux is required: pre.0 is built for {self.hidden}+{self.aux_dim} inputs (use_aux: true)")
        if tuple(aux.shape) != (fused.shape[0], self.aux_dim):
            raise RuntimeError(f"{what}: aux: expected ({fused.shape[0]},{self.aux_dim}), got {tuple(aux.shape)}")
        return fused, (aux if self.aux_dim else None)

    def _explain_device(self, what: str, *tensors: Optional[torch.Tensor]) -> torch.device:
        dev = self._arena.device
        if dev.type != "cuda":
            raise L.UltrafndHipError(f"DeepTruthClassifier.{what} runs on a HIP device only: call .to('cuda') (there is no CPU fallback)")
        L.require_hip(*tensors, self._arena.data)
        return dev

    XWS_KEEP_FLOATS = 1 << 24      # explanation workspaces up to 64 MiB stay on the module between calls; larger ones are the caller's

    def _explain_ws(self, rows: int) -> torch.Tensor:
        """A workspace of the explanations' own: `workspace(B, True)` keeps the activations of a pending backward.  The latest
        one is kept for the next call of the same size unless it is large (a 16 x 4,096-row smooth-grad pass needs about a
        gigabyte): that one is released when the call that asked for it drops it."""
        if self._xws is not None and self._xws[0] == rows:
            return self._xws[1]
        self._xws = None
        d = self.dims()
        n = L.lib().ufnd_clf_workspace_floats(C.byref(d), rows)
        ws = torch.empty(n, dtype=torch.float32, device=self._arena.device)
        if n <= self.XWS_KEEP_FLOATS:
            self._xws = (rows, ws)
        return ws

    def _input_grad(self, ws: torch.Tensor, fused_ptr: int, ld_fused: int, aux: Optional[torch.Tensor], rows: int, train: bool,
                    target: int, class_idx: int, gx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """ufnd_classifier_input_grad on `ws`.  Dropout masks (train) come from a step state of the explanations' own, advanced
        here: the module's state -- which a forward still waiting for its backward() relies on -- is never touched."""
        dev = self._arena.device
        if self._xrng is None:
            self._xrng = StepStateBuffer(dev, seed=torch.initial_seed() + 0xE7A)
        if train:
            self._xrng.advance()
        logits = torch.empty(rows, 2, dtype=torch.float32, device=dev)
        probs = torch.empty(rows, 2, dtype=torch.float32, device=dev)
        d = self.dims()
        L.check(L.lib().ufnd_classifier_input_grad(C.byref(d), C.byref(self.param_table()), fused_ptr, ld_fused, L.ptr(aux), rows,
                                                   int(bool(train)), target, class_idx, ws.data_ptr(), gx.data_ptr(), gx.stride(0),
                                                   logits.data_ptr(), probs.data_ptr(), self._xrng.ptr, L.stream_ptr(dev)),
                "ufnd_classifier_input_grad")
        return logits, probs

    def feature_importance(self, fused: torch.Tensor, aux: Optional[torch.Tensor] = None, class_idx: int = 1,
                           aggregate: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Gradient x input: (|d sum_b logits[b, class_idx] / dx * x| (B, F+A), its mean over the batch (F+A,) or None), x =
        cat[fused, aux] (:189-211).  Follows the module's mode (in train() the dropouts are live and two calls differ, as in the
        reference).  Device tensors; parameters, `.grad`, the module's step state and pending backwards are untouched.  The
        importances are computed in rows of hidden + 4 floats (the input panel's stride): unless F+A equals that, the returned
        (B, F+A) tensor is a view with that row stride -- `.contiguous()` it before handing its `data_ptr()` on."""
        if class_idx not in (0, 1):
            raise ValueError(f"feature_importance: class_idx={class_idx}: the head has two classes (0, 1)")
        fused, aux = self._explain_args(fused, aux, "feature_importance")
        B = fused.shape[0]
        if B > L.MAX_ROWS:
            raise ValueError(f"feature_importance: {B} rows: one call takes at most {L.MAX_ROWS}")
        dev = self._explain_device("feature_importance", fused, aux)
        fused = L.f32c(fused)
        aux = L.f32c(aux) if aux is not None else None
        if fused.data_ptr() % 16 != 0:
            fused = fused.clone()
        H, W, ld = self.hidden, self.hidden + self.eff_aux, self.hidden + 4
        ws = self._explain_ws(B)
        gx = torch.empty(B, ld, dtype=torch.float32, device=dev)
        self._input_grad(ws, fused.data_ptr(), fused.stride(0), aux, B, self.training, L.TARGET_LOGIT, class_idx, gx)
        d, ldx = self.dims(), C.c_int(0)
        xin = L.lib().ufnd_clf_input_panel(C.byref(d), ws.data_ptr(), B, C.byref(ldx))
        imp = torch.empty(B, ld, dtype=torch.float32, device=dev)
        agg = torch.empty(W, dtype=torch.float32, device=dev) if aggregate else None
        part = torch.empty(-(-B // L.ATTR_SLICE_ROWS) * W, dtype=torch.float32, device=dev) if aggregate else None
        L.check(L.lib().ufnd_attribution_reduce(L.ATTR_GRAD_X_INPUT, gx.data_ptr(), ld, xin, ldx.value, B, W, 1, 0, 0, imp.data_ptr(), ld,
                                                L.ptr(agg), L.ptr(part), L.stream_ptr(dev)), "ufnd_attribution_reduce")
        return imp[:, :W], agg

    def explain_shap(self, fused: torch.Tensor, aux: Optional[torch.Tensor] = None, max_samples: int = 256, *,
                     noise: Optional[torch.Tensor] = None) -> Dict[str, object]:
        """{"method": "smooth-grad", "values": np.float32 (min(B, max_samples), F+A)}: the reference's smooth-grad branch
        (:251-272; `shap` is never imported).  sigma = 0.1 std(X, rows).clamp_min(1e-6) of the unperturbed rows; the 16
        evaluation points are the reference's random WALK X_i = X_0 + sigma * sum_{j<i} n_j (the 16th draw is unused); values =
        mean_i |d sum_b probs[b, 1] / d X_i|.  `noise`: (16, B', F+A) draws used instead of torch.randn on the device.  Puts the
        module into eval mode and leaves it there, as the reference does.  All 16 B' rows run as one forward and one backward
        (in chunks of whole steps beyond 65,536 rows)."""
        N = self.SMOOTHGRAD_STEPS
        fused, aux = self._explain_args(fused, aux, "explain_shap")
        n = min(fused.shape[0], int(max_samples))
        if n < 2:
            raise ValueError(f"explain_shap: {n} row(s): sigma is the standard deviation over the batch rows, which needs B >= 2 "
                             "(the reference returns NaN for a single row)")
        if n > L.MAX_ROWS:
            raise ValueError(f"explain_shap: {n} rows: one step of the walk takes at most {L.MAX_ROWS} rows; lower max_samples")
        H, W, ld = self.hidden, self.hidden + self.eff_aux, self.hidden + 4
        if noise is not None and (not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (N, n, W)):
            raise ValueError(f"explain_shap: noise: expected ({N},{n},{W}), got {tuple(getattr(noise, 'shape', ()))}")
        dev = self._explain_device("explain_shap", fused, aux, noise)
        self.eval()
        # one-off plumbing on the device: X_0 = cat[fused, aux] and sigma in rows of hidden + 4 floats (the input panel's stride, so
        # that every strip of the walk is one 16-byte access).  A caller's noise is used where it lies when its rows are 16-byte
        # aligned (F+A a multiple of 4: no aux, or aux_dim 4); with aux_dim 2 (514 columns) it is copied once into padded rows.
        X = torch.zeros(n, ld, dtype=torch.float32, device=dev)
        X[:, :H] = fused[:n]
        if aux is not None:
            X[:, H:W] = aux[:n]
        sigma = torch.zeros(ld, dtype=torch.float32, device=dev)
        sigma[:W] = 0.1 * X[:, :W].std(dim=0).clamp_min(1e-6)
        if noise is None:
            nz = torch.randn(N, n, ld, dtype=torch.float32, device=dev)
        elif W % 4 == 0 and L.f32c(noise).data_ptr() % 16 == 0:
            nz = L.f32c(noise)
        else:
            nz = torch.zeros(N, n, ld, dtype=torch.float32, device=dev)
            nz[:, :, :W] = noise
        ldn = nz.stride(1)
        per = min(N, L.MAX_ROWS // n)                      # whole steps per call
        vals = torch.empty(n, ld, dtype=torch.float32, device=dev)
        lib, d, s = L.lib(), self.dims(), L.stream_ptr(dev)
        for step0 in range(0, N, per):
            steps = min(per, N - step0)
            rows = steps * n
            ws = self._explain_ws(rows)
            L.check(lib.ufnd_smoothgrad_points(C.byref(d), X.data_ptr(), ld, sigma.data_ptr(), nz.data_ptr(), ldn, n, N, step0, steps,
                                               ws.data_ptr(), s), "ufnd_smoothgrad_points")
            ldx = C.c_int(0)
            xin = lib.ufnd_clf_input_panel(C.byref(d), ws.data_ptr(), rows, C.byref(ldx))
            gx = torch.empty(rows, ld, dtype=torch.float32, device=dev)
            self._input_grad(ws, xin, ldx.value, None, rows, False, L.TARGET_PROB, 1, gx)
            L.check(lib.ufnd_attribution_reduce(L.ATTR_SMOOTHGRAD, gx.data_ptr(), ld, None, 0, n, W, steps, int(step0 > 0),
                                                N if step0 + steps == N else 0, vals.data_ptr(), ld, None, None, s), "ufnd_attribution_reduce")
        return {"method": "smooth-grad", "values": np.ascontiguousarray(vals[:, :W].cpu().numpy())}
