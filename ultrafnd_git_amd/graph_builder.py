"""The reference's post graph (src/models/gnn/graph_builder.py), MI355X-native.

Same four names, argument order and defaults:
  cosine_knn(X, k=8)                                       :4-28    symmetric cosine kNN graph with self-loops
  add_ocr_overlap_weights(A, ocr_sets, alpha=0.4)          :30-45   A[i][j] += alpha * log1p(|set_i & set_j|), in place
  add_temporal_inconsistency(A, delay_scores, beta=0.25)   :47-59   A[i][j] *= 1 + beta * |d_i - d_j|, in place
  build_dense_adj(X, ocr_sets, delay_scores, k, alpha, beta) :61-68 the three in a row
plus cosine_knn_indices(X, k) -> (N, k) int32, the sparse form of the kNN graph.

The reference runs three O(N^2) Python loops over a dense matrix.  Here the similarity matrix never exists: one C-ABI
call (ufnd_cosine_knn) normalises X and selects every row's k neighbours on chip, a second (ufnd_dense_adj) writes A
once, the kNN membership and both weightings in the same pass.  Inputs are np.ndarray or torch.Tensor; results are fp32
tensors on `device`.  There is no CPU path: a CPU tensor, a CPU `device=` or a missing library raises UltrafndHipError.

The neighbour selection orders by (similarity descending, index ascending).  The reference's np.argpartition leaves the
order among equal similarities open, and its float32 S differs from any other evaluation in the last bits, so a row whose
k-th and (k+1)-th similarities are closer than fp32 rounding may legitimately pick the other one.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib as L
from .gcn import sets_to_csr


def _device(device, *tensors) -> torch.device:
    """The device of the call: that of the tensor arguments (which must be HIP tensors), else `device`."""
    dev = L.require_hip(*[t for t in tensors if isinstance(t, torch.Tensor)])
    if dev is None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.UltrafndHipError("graph_builder runs on a HIP device only (no CPU fallback)")
    return dev


def _f32(x, dev: torch.device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(torch.float32)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(dev)


def _check_k(k, n: int) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1 or int(k) > L.KNN_MAX_K:
        raise ValueError(f"k={k!r}: an integer in 1..{L.KNN_MAX_K}")
    if int(k) >= n:
        raise ValueError(f"k={int(k)} needs k < N={n}: a row has N - 1 candidates (np.argpartition raises there too)")
    return int(k)


def _features(X, dev: torch.device) -> torch.Tensor:
    X = _f32(X, dev)
    if X.stride(1) != 1 or X.stride(0) < X.shape[1]:       # a row-strided view (ldx > D) is read in place
        X = X.contiguous()
    return X


def _square(A) -> torch.Tensor:
    if not isinstance(A, torch.Tensor):
        raise L.UltrafndHipError("A must be a tensor on a HIP device: it is updated in place (no CPU fallback)")
    L.require_hip(A)
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float32 or A.stride(1) != 1 or A.stride(0) < A.shape[1]:
        raise ValueError(f"A {tuple(A.shape)} {A.dtype}: expected a square fp32 matrix with unit column stride")
    return A


def _csr(ocr_sets: Sequence[set], n: int, dev: torch.device):
    if len(ocr_sets) != n:
        raise ValueError(f"{len(ocr_sets)} phrase sets for {n} nodes")
    offs, toks = sets_to_csr(ocr_sets)
    return torch.from_numpy(offs).to(dev), torch.from_numpy(toks if toks.size else np.zeros(1, dtype=np.int32)).to(dev)


def _delay(delay_scores, n: int, dev: torch.device) -> torch.Tensor:
    d = _f32(delay_scores, dev).to(dev).reshape(-1).contiguous()
    if d.numel() != n:
        raise ValueError(f"{d.numel()} delay scores for {n} nodes")
    return d


def _dense_adj(idx, k, csr, delay, alpha, beta, adj: torch.Tensor, flags: int) -> torch.Tensor:
    offs, toks = csr if csr is not None else (None, None)
    L.check(L.lib().ufnd_dense_adj(L.ptr(idx), int(k), L.ptr(offs), L.ptr(toks), L.ptr(delay), float(alpha), float(beta), adj.shape[0],
                                   adj.data_ptr(), adj.stride(0), flags, L.stream_ptr(adj.device)), "ufnd_dense_adj")
    return adj


def cosine_knn_indices(X, k: int = 8, device="cuda") -> torch.Tensor:
    """(N, k) int32: row i's k nearest rows of X (N, D) by cosine similarity, i excluded, ordered by (similarity descending,
    index ascending).  Rows are divided by (norm + 1e-9) in fp32 and S = Xn Xn^T is accumulated in exact fp32; S is never
    stored.  Two calls give identical bits.  k >= N raises ValueError, as NumPy's argpartition does."""
    dev = _device(device, X)
    shape = tuple(X.shape) if hasattr(X, "shape") else np.shape(X)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"X {shape}: expected (N, D)")
    k = _check_k(k, shape[0])          # (before anything touches the device)
    X = _features(X, dev)
    n, d = X.shape
    ws = torch.empty(L.lib().ufnd_cosine_knn_workspace_floats(n, d, k), dtype=torch.float32, device=dev)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    L.check(L.lib().ufnd_cosine_knn(X.data_ptr(), X.stride(0), n, d, k, idx.data_ptr(), ws.data_ptr(), L.stream_ptr(dev)),
            "ufnd_cosine_knn")
    return idx


def cosine_knn(X, k: int = 8, device="cuda") -> torch.Tensor:
    """(N, N) fp32 symmetric kNN graph with unit diagonal: A[i][j] = 1 where j is among i's k nearest or i among j's."""
    idx = cosine_knn_indices(X, k, device=device)
    adj = torch.empty(idx.shape[0], idx.shape[0], dtype=torch.float32, device=idx.device)
    return _dense_adj(idx, k, None, None, 0.0, 0.0, adj, L.ADJ_KNN)


def add_ocr_overlap_weights(A: torch.Tensor, ocr_sets: Sequence[set], alpha: float = 0.4) -> torch.Tensor:
    """A[i][j] += alpha * log1p(|set_i & set_j|) for i != j with a non-empty intersection, evaluated as the reference's NumPy
    does: (float)((double)a + alpha * log1p(ov)).  Mutates A (a square fp32 HIP tensor) and returns it, as the reference does."""
    A = _square(A)
    return _dense_adj(None, 0, _csr(ocr_sets, A.shape[0], A.device), None, alpha, 0.0, A, L.ADJ_OCR)


def add_temporal_inconsistency(A: torch.Tensor, delay_scores, beta: float = 0.25) -> torch.Tensor:
    """A[i][j] *= 1 + beta * |d_i - d_j| for i != j, every operation rounded to fp32 as NumPy does on a float32 array.
    `delay_scores` is converted to fp32 on entry: given a float64 array the reference computes the factor in double, so the
    result here may differ from it in the last fp32 bit.  Mutates A and returns it."""
    A = _square(A)
    return _dense_adj(None, 0, None, _delay(delay_scores, A.shape[0], A.device), 0.0, beta, A, L.ADJ_TEMPORAL)


def build_dense_adj(X, ocr_sets: Sequence[set], delay_scores, k: int = 8, alpha: float = 0.4, beta: float = 0.25,
                    device="cuda") -> torch.Tensor:
    """cosine_knn, add_ocr_overlap_weights and add_temporal_inconsistency in a row, as two C-ABI calls: the neighbour
    selection, then ONE pass that writes A -- bit for bit what the three separate calls give.  `delay_scores` as for
    add_temporal_inconsistency (fp32 on entry)."""
    idx = cosine_knn_indices(X, k, device=device)
    n, dev = idx.shape[0], idx.device
    csr, delay = _csr(ocr_sets, n, dev), _delay(delay_scores, n, dev)
    adj = torch.empty(n, n, dtype=torch.float32, device=dev)
    return _dense_adj(idx, k, csr, delay, alpha, beta, adj, L.ADJ_KNN | L.ADJ_OCR | L.ADJ_TEMPORAL)
