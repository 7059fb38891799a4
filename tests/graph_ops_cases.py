"""Cases, float64 references, bounds, float32 restatements and mutants of the graph side and the temporal side:
csrc/gcn.hip (ufnd_gcn_forward, ufnd_gcn_pretrain_step, ufnd_gnn_forward, ufnd_gnn_backward, ufnd_node_features, both OCR
adjacencies), csrc/tcn.hip (ufnd_tcn_forward) and csrc/temporal.hip (ufnd_temporal_align).  Shared by
tests/test_graph_ops_cases.py (CPU: every restatement stays inside its bound and is bit-equal on the exact families, every
mutant leaves a bound by MUTANT_FACTOR, the table reaches every class) and tests/test_gpu_graph_ops.py (GPU: every case
through the C ABI against float64).  The layout is that of tests/frozen_ops_cases.py and tests/step_tail_cases.py, whose U,
HW_ULP, MUTANT_FACTOR and worst_ratio are used here.

An entry is an `Op`: `cases`, `make(case) -> inputs`, `restate(case, inputs, dt, mutant=None, muls=None) -> {output: array}`
-- ONE plain NumPy statement of the operation, run in float64 for the reference and in float32 for the restatement -- and the
names of its mutants.  `reference(op, case, inputs)` returns {output: (ref float64, bound)}.

Bounds.
  exact           integer results and the exact families (`is_exact(op, case)`): bound 0, bit equality.
  derived         ufnd_node_features, one kernel: out = v * (1 / (sqrtf(ss) + 1e-9f)).  Every lane adds ceil(F / 64) squares in
                  sequence and the wave's butterfly adds six levels: the sum of the (rounded, one u each) positive squares is
                  within (ceil(F / 64) + 7) u of itself and the square root halves that; sqrtf 2 u (1 ulp, HIP's table), the
                  float32 constant 1e-9f and the addition one u each, the division 5 u (2.5 ulp), the product one u:
                  |err| <= |ref| ((ceil(F / 64) + 7) / 2 + 10) u (1 + 1e-3).  A zero row gives exact zeros.
  mirror-relative composite entries (GCN / GNN forward, backward and pretrain step, ufnd_temporal_align, the TCN): the rule of the
                  audio and CLIP-text tests.  max|gpu - ref64| of an output must stay within BOUND_FACTOR = 3 times
                  max|restatement32 - ref64| of that output on that same input.  The restatement keeps the kernels' operation order
                  where it matters (the two-pass variance, the pooling order, powf(s + 1 + 1e-9f, -0.5f), (dinv_i a_ij) dinv_j);
                  its matrix products are NumPy's.  Nothing is bounded by what the kernels produce.
  the loss        of ufnd_gcn_pretrain_step is ONE number per case: a single rounding-error draw against another single draw says
                  nothing at a factor of 3 (two equal Gaussians differ by more than that once in five).  The loss is therefore
                  judged as one output over the whole pretrain table: max over the cases of |gpu - ref| / |ref| within
                  BOUND_FACTOR times the same maximum of the restatement (loss_table_ratio).
  the ReLU kink   a gate [U > 0] of GNNModel may flip where |U| in float64 is below the forward bound of U; the gradient rows it
                  feeds (row h of g_w1, g_b1[h] for a flipped U[:, h]) are excluded, at most KINK_CAP = 1 % of a case's gradient
                  elements.  The seeds are chosen so that no case of the table excludes anything; the CPU test asserts the cap.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, NamedTuple, Tuple

import numpy as np
import torch

from tests.frozen_ops_cases import HW_ULP, MUTANT_FACTOR, U, _seed, worst_ratio  # noqa: F401

BOUND_FACTOR = 3.0
KINK_CAP = 0.01
F64, F32 = np.float64, np.float32

# dropout stream tags (csrc/gcn.hip LAYER_GNN, csrc/tcn.hip LAYER_TCN + layer)
LAYER_GNN, LAYER_TCN = 10, 16
DROP_P = 0.1
DROP_SEED, DROP_STEP = 0x5EED1234, 7


class Op(NamedTuple):
    cases: List[tuple]
    make: Callable
    restate: Callable
    mutants: Tuple[str, ...] = ()


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gelu(x):
    dt = x.dtype.type
    return dt(0.5) * x * (dt(1) + _erf(x * dt(0.70710678118654752440)))


def gelu_grad(x):
    dt = x.dtype.type
    cdf = dt(0.5) * (dt(1) + _erf(x * dt(0.70710678118654752440)))
    return cdf + x * (dt(0.39894228040143267794) * np.exp(dt(-0.5) * x * x))


# ---------------------------------------------------------------------------------------------------------------------
# graphs
SYMMETRIC = ("empty", "complete", "star", "unit_diag", "zero_diag", "weighted_sym")
DIRECTED = ("ring_directed", "random_directed", "weighted_asym")
KINDS = SYMMETRIC + DIRECTED
GRAPH_N = (1, 2, 31, 32, 33, 64, 65, 257)


def make_adj(kind: str, N: int, seed: int) -> np.ndarray:
    rng = _seed(11, N, seed)
    a = np.zeros((N, N), dtype=F64)
    off = ~np.eye(N, dtype=bool)
    if kind == "complete":
        a[off] = 1.0
    elif kind == "star":
        a[0, 1:] = 1.0
        a[1:, 0] = 1.0
    elif kind in ("unit_diag", "zero_diag"):
        r = np.triu(rng.random((N, N)) < 0.1, 1)
        a = (r | r.T).astype(F64)
        if kind == "unit_diag":
            np.fill_diagonal(a, 1.0)
    elif kind == "weighted_sym":
        r = np.triu((rng.random((N, N)) < 0.2) * (1.0 - rng.random((N, N))), 1)      # weights in (0, 1]
        a = r + r.T
    elif kind == "ring_directed":
        if N > 1:
            a[np.arange(N), (np.arange(N) + 1) % N] = 1.0
    elif kind == "random_directed":
        a = ((rng.random((N, N)) < 0.1) & off).astype(F64)
    elif kind == "weighted_asym":
        a = (rng.random((N, N)) < 0.2) * (1.0 - rng.random((N, N))) * off
    elif kind != "empty":
        raise KeyError(kind)
    return np.ascontiguousarray(a, dtype=F32)


def norm_adj(adj, dt, flavour, mutant=None):
    """A_norm = D^-1/2 (adj + I) D^-1/2.  float32: gcn_degree_kernel's powf(s + 1 + 1e-9f, -0.5f) and gcn_norm_adj_kernel's
    (dinv_i (a_ij + [i == j])) dinv_j.  float64: SimpleGCN adds 1e-9 to the degree, GNNModel clamps it at 1e-9."""
    a = adj.astype(dt)
    N = a.shape[0]
    s = a.sum(axis=1)
    one = dt(0) if mutant == "degree_without_plus_one" else dt(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if dt is F32:
            dinv = np.power(s + one + F32(1e-9), F32(-0.5))
        elif flavour == "gcn":
            dinv = (s + one + 1e-9) ** -0.5
        else:
            dinv = np.maximum(s + one, 1e-9) ** -0.5
        return (dinv[:, None] * (a + np.eye(N, dtype=dt))) * dinv[None, :], s


def aggregate(A, H, mutant):
    """A (N, N) times H (N, hid).  The kernels run it as an (N, Np) x (Np, hid) product, Np = N rounded up to 32, whose pad rows
    must be zero: the mutant leaves them as they were (NaN in a poisoned workspace)."""
    N = A.shape[0]
    Np = (N + 31) & ~31
    if mutant == "pad_rows_not_zeroed" and Np > N:
        Ap = np.concatenate([A, np.zeros((N, Np - N), dtype=A.dtype)], axis=1)
        Hp = np.concatenate([H, np.full((Np - N, H.shape[1]), np.nan, dtype=H.dtype)], axis=0)
        with np.errstate(invalid="ignore"):
            return Ap @ Hp
    return A @ H


def _widths(i, j):
    return (4, 20)[(i + j) % 2], (32, 96)[((i + j) // 2) % 2], 32


def _graph_table():
    out = []
    for i, N in enumerate(GRAPH_N):
        for j, kind in enumerate(KINDS):
            F, hid, od = _widths(i, j)
            out.append((N, kind, F, hid, od, 3 * ((i + (j + 1) // 2) % 2)))      # ld_adj = N or N + 3
    return out


def _gcn_inputs(rng, N, kind, F, hid, od, integers=False):
    if integers:
        draw = lambda *s: rng.integers(-2, 3, size=s).astype(F32)
        w1, w2 = rng.integers(-1, 2, size=(hid, F)).astype(F32), rng.integers(-1, 2, size=(od, hid)).astype(F32)
        return {"x": draw(N, F), "w1": w1, "b1": rng.integers(-1, 2, size=hid).astype(F32), "w2": w2, "b2": rng.integers(-1, 2, size=od).astype(F32),
                "d_z": draw(N, od)}
    g = lambda *s: rng.standard_normal(s)
    return {"x": g(N, F).astype(F32), "w1": (g(hid, F) / math.sqrt(F)).astype(F32), "b1": (0.5 * g(hid)).astype(F32),
            "w2": (g(od, hid) / math.sqrt(hid)).astype(F32), "b2": (0.1 * g(od)).astype(F32), "d_z": g(N, od).astype(F32)}


# ---------------------------------------------------------------------------------------------------------------------
# GNNModel forward + backward.  case = (N, kind, in_dim, hid, out, ld_extra, family); family in normal / exact / relu_zero / dropout
GNN_EXACT_N = GRAPH_N
GNN_DROP = [(33, "weighted_sym"), (33, "random_directed"), (64, "zero_diag"), (64, "weighted_asym")]


def _gnn_cases():
    out = [c + ("normal",) for c in _graph_table()]
    out += [(N, "empty", (4, 20)[i % 2], (32, 96)[i % 2], 32, 3 * (i % 2), "exact") for i, N in enumerate(GNN_EXACT_N)]
    out += [(N, "random_directed", 20, 32, 32, 0, "relu_zero") for N in (33, 64)]
    out += [(N, kind, 20, 96, 32, 3, "dropout") for N, kind in GNN_DROP]
    return out


def _gnn_make(case):
    N, kind, F, hid, od, ldx, fam = case
    rng = _seed(21, N, KINDS.index(kind), F, hid, ("normal", "exact", "relu_zero", "dropout").index(fam))
    inp = _gcn_inputs(rng, N, kind, F, hid, od, integers=fam in ("exact", "relu_zero"))
    if fam == "relu_zero":
        inp["w1"][:] = 0
        inp["b1"][:] = 0
    inp["adj"] = make_adj(kind, N, 1)
    return inp


def gnn_muls(case, step=DROP_STEP, ld=None, tag=LAYER_GNN):
    from tests import dropout_mirror as DM
    N, hid = case[0], case[3]
    return DM.multipliers(DROP_SEED, step, tag, DROP_P, N, hid, hid if ld is None else ld)


def _gnn_restate(case, inp, dt, mutant=None, muls=None):
    x, w1, b1, w2, b2, dz = (inp[k].astype(dt) for k in ("x", "w1", "b1", "w2", "b2", "d_z"))
    An, _ = norm_adj(inp["adj"], dt, "gnn", mutant)
    AnT = An if mutant == "an_not_transposed" else np.ascontiguousarray(An.T)
    mul = dt(1) if muls is None else muls.astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        Y1 = x @ w1.T + b1
        Uh = aggregate(An, Y1, mutant)
        H = np.maximum(Uh, dt(0)) * mul
        G = aggregate(An, H, mutant)
        Z = G @ w2.T + b2
        dG = dz @ w2
        dH = aggregate(AnT, dG, mutant)
        gate = (Uh >= 0) if mutant == "relu_ge_zero" else (Uh > 0)
        dU = np.where(gate, dH, dt(0)) * mul
        dY1 = aggregate(AnT, dU, mutant)
        return {"z": Z, "g_w1": dY1.T @ x, "g_b1": dY1.sum(axis=0), "g_w2": dz.T @ G, "g_b2": dz.sum(axis=0), "_U": Uh}


# ---------------------------------------------------------------------------------------------------------------------
# SimpleGCN forward and the pretrain step.  case = (N, kind, in_dim, hid, out, ld_extra, variant)
GCN_VARIANTS = ("step1", "step2", "step1000", "weight_decay", "saturated_high", "saturated_low")
GCN_LR = 1e-2


def _gcn_cases():
    out = [c + ("step1",) for c in _graph_table()]
    for v in GCN_VARIANTS[1:]:
        out += [(33, "random_directed", 20, 96, 32, 3, v), (64, "weighted_sym", 4, 32, 32, 0, v)]
    return out


def _gcn_make(case):
    N, kind, F, hid, od, ldx, variant = case
    rng = _seed(31, N, KINDS.index(kind), F, hid, GCN_VARIANTS.index(variant))
    inp = _gcn_inputs(rng, N, kind, F, hid, od)
    del inp["d_z"]
    inp["adj"] = make_adj(kind, N, 2)
    inp["head_w"] = (rng.standard_normal(od) / math.sqrt(od)).astype(F32)
    inp["head_b"] = np.array([{"saturated_high": 100.0, "saturated_low": -100.0}.get(variant, 0.1)], dtype=F32)
    n = hid * F + hid + od * hid + od
    fresh = variant in ("step1", "weight_decay", "saturated_high", "saturated_low")
    inp["m"] = np.zeros(n, dtype=F32) if fresh else (1e-3 * rng.standard_normal(n)).astype(F32)
    inp["v"] = np.zeros(n, dtype=F32) if fresh else (1e-6 * rng.random(n)).astype(F32)
    inp["step"] = {"step2": 2, "step1000": 1000}.get(variant, 1)
    inp["wd"] = 0.05 if variant == "weight_decay" else 0.0
    return inp


def _gcn_restate(case, inp, dt, mutant=None, muls=None):
    N = case[0]
    x, w1, b1, w2, b2, wh, bh = (inp[k].astype(dt) for k in ("x", "w1", "b1", "w2", "b2", "head_w", "head_b"))
    An, rowsum = norm_adj(inp["adj"], dt, "gcn", mutant)
    AnT = An if mutant == "an_not_transposed" else np.ascontiguousarray(An.T)
    mul = dt(1) if muls is None else muls.astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        P = aggregate(An, x, mutant)
        U1 = P @ w1.T + b1
        H = gelu(U1) * mul
        Q = aggregate(An, H, mutant)
        Z = Q @ w2.T + b2
        s = Z @ wh + bh[0]
        pred = dt(1) / (dt(1) + np.exp(-s))
        t = (rowsum + (dt(1) if mutant == "target_over_adj_plus_I" else dt(0))) / dt(max(1, N))
        d = pred - t
        loss = (d * d / dt(N)).sum()
        dZ = (dt(2) * d / dt(N) * pred * (dt(1) - pred))[:, None] * wh[None, :]
        dQ = dZ @ w2
        dU1 = aggregate(AnT, dQ, mutant) * gelu_grad(U1) * mul
        g = np.concatenate([(dU1.T @ P).ravel(), dU1.sum(axis=0), (dZ.T @ Q).ravel(), dZ.sum(axis=0)])
        p = np.concatenate([w1.ravel(), b1, w2.ravel(), b2])
        m, v = inp["m"].astype(dt), inp["v"].astype(dt)
        lr, wd, be1, be2, step = dt(GCN_LR), dt(inp["wd"]), dt(0.9), dt(0.999), inp["step"]
        if dt is F32:      # the launcher's host arithmetic: float powf
            bc1 = F32(1) - F32(math.pow(float(be1), step))
            bc2s = np.sqrt(F32(1) - F32(math.pow(float(be2), step)))
        else:
            bc1, bc2s = 1.0 - 0.9 ** step, math.sqrt(1.0 - 0.999 ** step)
        if mutant == "adamw_decoupled_decay":
            p = p * (dt(1) - lr * wd)
        else:
            g = g + wd * p
        m = be1 * m + (dt(1) - be1) * g
        v = be2 * v + (dt(1) - be2) * g * g
        p = p - (lr / bc1) * m / (np.sqrt(v) / bc2s + dt(1e-8))
    return {"z": Z, "loss": np.asarray([loss]), "params": p, "exp_avg": m, "exp_avg_sq": v}


# ---------------------------------------------------------------------------------------------------------------------
# ufnd_node_features.  case = (widths, B, row kinds)
NF_WIDTHS = ((1, 1, 1, 1), (3, 5, 7, 2), (192, 64, 96, 64))
NF_LD_EXTRA = (3, 1, 5, 2)


def _nf_cases():
    return [(w, B) for w in NF_WIDTHS for B in (1, 4, 5)]


def _nf_make(case):
    w, B = case
    rng = _seed(41, sum(w), B)
    parts = [rng.standard_normal((B, n)).astype(F32) for n in w]
    if B >= 4:
        for p in parts:
            p[1] = 0.0                                                    # a zero row
        scale = 1e-10 / math.sqrt(sum(float((p[2].astype(F64) ** 2).sum()) for p in parts))
        for p in parts:
            p[2] = (p[2] * scale).astype(F32)                             # a row of norm 1e-10: the eps decides
    return {"parts": parts}


def _nf_restate(case, inp, dt, mutant=None, muls=None):
    v = np.concatenate([p.astype(dt) for p in inp["parts"]], axis=1)
    nrm = np.sqrt((v * v).sum(axis=1, keepdims=True))
    den = np.maximum(nrm, dt(1e-9)) if mutant == "norm_max_eps" else nrm + dt(1e-9)
    return {"out": v * (dt(1) / den)}


def nf_bound(case, ref):
    F = sum(case[0])
    return np.abs(ref) * ((math.ceil(F / 64) + 7) / 2 + 10) * U * (1 + 1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# ufnd_temporal_align (eval).  case = (D, Dv, B); hidden 64, out 32
TA_D = (1, 2, 3, 64, 65)
TA_HIDDEN, TA_OUT = 64, 32
TA_ROWS = ("normal", "zero_text", "zero_visual", "both_zero", "identical", "tiny")


def _ta_cases():
    out = []
    for i, D in enumerate(TA_D):
        dvs = sorted({1, D, D + 2} | ({D - 1} if D > 1 else set()))
        for j, Dv in enumerate(dvs):
            out.append((D, Dv, (1, 4, 5)[(i + j) % 3]))
    out += [(64, 64, 5), (65, 40, 4), (3, 3, 5)]
    return sorted(set(out))


def ta_row_kinds(B):
    return {1: ("normal",), 4: ("both_zero", "identical", "tiny", "normal"), 5: TA_ROWS[1:]}[B]


def _ta_make(case):
    D, Dv, B = case
    rng = _seed(51, D, Dv, B)
    t, v = rng.standard_normal((B, D)).astype(F32), rng.standard_normal((B, Dv)).astype(F32)
    for r, kind in enumerate(ta_row_kinds(B)):
        if kind in ("zero_text", "both_zero"):
            t[r] = 0
        if kind in ("zero_visual", "both_zero"):
            v[r, :D] = 0
        if kind == "identical":
            n = min(D, Dv)
            v[r] = 0
            v[r, :n] = t[r, :n]
        if kind == "tiny":
            t[r] = (t[r] * (1e-10 / max(1e-30, float(np.linalg.norm(t[r].astype(F64)))))).astype(F32)
            n = min(D, Dv)
            v[r, :n] = (v[r, :n] * (1e-10 / max(1e-30, float(np.linalg.norm(v[r, :n].astype(F64)))))).astype(F32)
    hid, od, K = TA_HIDDEN, TA_OUT, 4 * D + 1
    w0 = (rng.standard_normal((hid, K)) / math.sqrt(K)).astype(F32)
    w0[:, 4 * D] = rng.standard_normal(hid).astype(F32)                     # the cosine's column weighs as much as all the others
    return {"t": t, "v": v, "w0": w0, "b0": (0.1 * rng.standard_normal(hid)).astype(F32),
            "w3": (rng.standard_normal((od, hid)) / math.sqrt(hid)).astype(F32), "b3": (0.1 * rng.standard_normal(od)).astype(F32)}


def _ta_restate(case, inp, dt, mutant=None, muls=None):
    D, Dv, B = case
    t = inp["t"].astype(dt)
    v = np.zeros((B, D), dtype=dt)
    n = min(D, Dv)
    v[:, :n] = inp["v"][:, :n].astype(dt)
    tt, vv, tv = (t * t).sum(axis=1), (v * v).sum(axis=1), (t * v).sum(axis=1)
    eps = dt(1e-9)
    if mutant == "cosine_max_eps":
        cos = tv / (np.maximum(np.sqrt(tt), eps) * np.maximum(np.sqrt(vv), eps))
    else:
        cos = tv / ((np.sqrt(tt) + eps) * (np.sqrt(vv) + eps))
    if mutant == "visual_not_truncated_in_cosine":
        vv2 = (inp["v"].astype(dt) ** 2).sum(axis=1)
        cos = tv / ((np.sqrt(tt) + eps) * (np.sqrt(vv2) + eps))
    feat = np.concatenate([t, v, t - v, t * v, cos[:, None]], axis=1)
    h = gelu(feat @ inp["w0"].astype(dt).T + inp["b0"].astype(dt))
    return {"out": h @ inp["w3"].astype(dt).T + inp["b3"].astype(dt), "_cos": cos}


# ---------------------------------------------------------------------------------------------------------------------
# ufnd_tcn_forward.  case = (text_dim, vis_dim, hid, kernel, layers, T, B, mode, edge); mode in eval / train / dropout
TCN_OUT = 32
TCN_MOMENTUM, TCN_EPS = 0.1, 1e-5
TCN_CASES = [
    (3, 2, 32, 3, 4, 5, 3, "eval", None),          # C k = 15: padded weight stride; every off-centre tap of layers 2, 3 outside the clip
    (3, 2, 32, 2, 4, 33, 3, "eval", None),         # even kernel: the split of 'same' depends on the dilation
    (3, 2, 96, 4, 6, 33, 1, "eval", None),         # dilation 32, T = 33
    (16, 16, 32, 3, 4, 33, 3, "eval", None),       # C == hid: residual and concat at block 0
    (16, 16, 32, 1, 1, 1, 3, "eval", None),        # kernel 1, T = 1: mean == max
    (40, 24, 32, 15, 4, 5, 1, "eval", None),       # C > hid, kernel 15
    (40, 24, 96, 4, 6, 2, 3, "eval", None),
    (3, 2, 32, 15, 6, 33, 3, "eval", None),
    (3, 2, 32, 3, 1, 33, 3, "eval", "negative"),   # every activation into the max-pool negative
    (3, 2, 32, 3, 4, 2, 1, "train", None),         # M = 2
    (3, 2, 96, 2, 1, 1, 3, "train", None),         # M = 3
    (16, 16, 32, 4, 4, 5, 3, "train", None),
    (40, 24, 96, 3, 6, 33, 3, "train", None),
    (3, 2, 96, 3, 4, 33, 3, "train", "constant"),  # a channel made constant by a zero weight row
    (3, 2, 32, 3, 1, 33, 3, "train", "offset"),    # a channel with bias 300 and unit spread
    (3, 2, 32, 3, 6, 5, 3, "dropout", None),       # six layers: tag 21
    (16, 16, 96, 3, 4, 33, 1, "dropout", None),
]


def _tcn_make(case):
    td, vd, hid, k, layers, T, B, mode, edge = case
    rng = _seed(61, td, vd, hid, k, layers, T, B, ("eval", "train", "dropout").index(mode), (None, "negative", "constant", "offset").index(edge))
    g = lambda *s: rng.standard_normal(s)
    inp = {"text": g(B, T, td).astype(F32), "vis": g(B, T, vd).astype(F32), "layers": []}
    ch = td + vd
    for i in range(layers):
        L = {"w": (g(hid, k, ch) / math.sqrt(k * ch)).astype(F32), "b": (0.1 * g(hid)).astype(F32), "gamma": (1.0 + 0.2 * g(hid)).astype(F32),
             "beta": (0.1 * g(hid)).astype(F32), "rm": (0.1 * g(hid)).astype(F32), "rv": (0.5 + rng.random(hid)).astype(F32)}
        if i == 0 and edge == "constant":
            L["w"][5] = 0.0
        if i == 0 and edge == "offset":
            L["w"][7] *= math.sqrt(k * ch) / math.sqrt(k)            # unit spread
            L["b"][7] = 300.0
        if edge == "negative":
            L["gamma"][:], L["beta"][:] = 0.05, -1.0
        inp["layers"].append(L)
        ch = hid
    inp["head_w"] = (g(TCN_OUT, 2 * hid) / math.sqrt(2 * hid)).astype(F32)
    inp["head_b"] = (0.1 * g(TCN_OUT)).astype(F32)
    return inp


def tcn_muls(case, step=DROP_STEP, ld=None, shift=0):
    from tests import dropout_mirror as DM
    td, vd, hid, k, layers, T, B = case[:7]
    return [DM.multipliers(DROP_SEED, step, LAYER_TCN + i + shift, DROP_P, B * T, hid, hid if ld is None else ld) for i in range(layers)]


def _tcn_restate(case, inp, dt, mutant=None, muls=None):
    td, vd, hid, k, layers, T, B, mode, edge = case
    h = np.concatenate([inp["text"], inp["vis"]], axis=2).astype(dt).reshape(B * T, td + vd)
    M = B * T
    train = mode != "eval"
    out = {}
    tpos = np.arange(M) % T
    for i, L in enumerate(inp["layers"]):
        w = L["w"].astype(dt)
        d = 1 << i
        total = d * (k - 1)
        left = total - total // 2 if mutant == "right_heavy_padding" else total // 2
        y = np.broadcast_to(L["b"].astype(dt), (M, hid)).copy()
        for j in range(k):
            s = j * d - left
            src = np.arange(M) + s
            ok = (src >= 0) & (src < M) if mutant == "taps_wrap_into_the_next_clip" else (tpos + s >= 0) & (tpos + s < T)
            if ok.any():
                y[ok] += h[src[ok]] @ w[:, j, :].T
        if train:
            mean = y.sum(axis=0) / dt(M)
            if mutant == "one_pass_variance":
                var = np.maximum((y * y).sum(axis=0) / dt(M) - mean * mean, dt(0))
                ss = var * dt(M)
            else:
                ss = ((y - mean) ** 2).sum(axis=0)
                var = ss / dt(M)
            mom = dt(TCN_MOMENTUM)
            out[f"running_mean{i}"] = (dt(1) - mom) * L["rm"].astype(dt) + mom * mean
            out[f"running_var{i}"] = (dt(1) - mom) * L["rv"].astype(dt) + mom * (var if mutant == "running_var_biased" else ss / dt(M - 1))
        else:
            mean, var = L["rm"].astype(dt), L["rv"].astype(dt)
        z = gelu((y - mean) * (dt(1) / np.sqrt(var + dt(TCN_EPS))) * L["gamma"].astype(dt) + L["beta"].astype(dt))
        if muls is not None:
            z = z * muls[i].astype(dt)
        h = h + z if h.shape[1] == hid else z
    hb = h.reshape(B, T, hid)
    mean_t = np.zeros((B, hid), dtype=dt)
    for t in range(T):                                            # the kernel's order: frame by frame
        mean_t = mean_t + hb[:, t]
    mx = np.maximum(hb.max(axis=1), dt(0)) if mutant == "max_starts_at_zero" else hb.max(axis=1)
    pooled = np.concatenate([mean_t / dt(T), mx], axis=1)
    out["out"] = pooled @ inp["head_w"].astype(dt).T + inp["head_b"].astype(dt)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the OCR adjacencies (bit-exact): sets at the LDS window's edge and a Jaccard of exactly 1 / 3 at thresh = 1 / 3
ADJ_N = (256, 257)
ADJ_THRESH = 1.0 / 3.0


def adjacency_sets(N):
    """set 0: exactly 2048 phrases (the LDS window, full); set 1: 2049 (read from memory); set 2 overlaps both; sets 3 and 4: Jaccard
    exactly 1 / 3; set 5 empty; the rest small and random."""
    rng = np.random.RandomState(N)
    sets = [set(range(2048)), set(range(2049)), set(range(1000, 3049)), {5000, 5001}, {5001, 5002}, set()]
    while len(sets) < N:
        sets.append(set(int(t) for t in rng.randint(0, 40, size=int(rng.randint(1, 9)))))
    return sets[:N]


def adjacency_refs(sets, thresh):
    """(unweighted, weighted) in Python floats, as the reference's two loops (forensic_trainer.py:114-132, _integrated.py:77-98)."""
    n = len(sets)
    a, w = np.eye(n, dtype=F32), np.zeros((n, n), dtype=F32)
    for i in range(n):
        for j in range(i + 1, n):
            si, sj = sets[i], sets[j]
            inter = len(si & sj)
            union = len(si) + len(sj) - inter
            jac = inter / (union + 1e-9) if (si or sj) else 0.0
            if jac >= thresh:
                a[i, j] = a[j, i] = 1.0
            if si and sj and inter / union >= thresh:
                w[i, j] = w[j, i] = inter / union
    return a, w


# ---------------------------------------------------------------------------------------------------------------------
OPS: Dict[str, Op] = {
    "gnn": Op(_gnn_cases(), _gnn_make, _gnn_restate, ("an_not_transposed", "degree_without_plus_one", "relu_ge_zero", "pad_rows_not_zeroed")),
    "gcn_pretrain": Op(_gcn_cases(), _gcn_make, _gcn_restate,
                       ("an_not_transposed", "degree_without_plus_one", "target_over_adj_plus_I", "adamw_decoupled_decay", "pad_rows_not_zeroed")),
    "node_features": Op(_nf_cases(), _nf_make, _nf_restate, ("norm_max_eps",)),
    "temporal_align": Op(_ta_cases(), _ta_make, _ta_restate, ("cosine_max_eps", "visual_not_truncated_in_cosine")),
    "tcn": Op(TCN_CASES, _tcn_make, _tcn_restate,
              ("right_heavy_padding", "taps_wrap_into_the_next_clip", "running_var_biased", "one_pass_variance", "max_starts_at_zero")),
}
GCN_EXACT_OUTPUTS = ("params", "exp_avg", "exp_avg_sq")      # of the saturated head: every gradient and moment 0, the parameters keep their bits


def case_id(case) -> str:
    return "-".join("x".join(map(str, c)) if isinstance(c, tuple) else str(c) for c in case)


def is_exact(op, case) -> bool:
    return op == "gnn" and case[6] in ("exact", "relu_zero")


def case_muls(op, case, **kw):
    """The dropout multipliers a train-mode case runs with (None: no dropout)."""
    if op == "gnn" and case[6] == "dropout":
        return gnn_muls(case, **kw)
    if op == "tcn" and case[7] == "dropout":
        return tcn_muls(case, **kw)
    return None


def reference(op, case, inp, muls="own") -> Dict[str, tuple]:
    """{output: (ref float64, bound)}; gradient exclusions of the ReLU kink under "_excluded" (g_w1 rows / g_b1 entries)."""
    o = OPS[op]
    muls = case_muls(op, case) if isinstance(muls, str) else muls
    ref = o.restate(case, inp, F64, None, muls)
    if op == "node_features":
        return {"out": (ref["out"], nf_bound(case, ref["out"]))}
    mir = o.restate(case, inp, F32, None, muls)
    out = {}
    for k in ref:
        if k.startswith("_"):
            continue
        if is_exact(op, case):
            b = 0.0
        else:
            b = BOUND_FACTOR * float(np.max(np.abs(mir[k].astype(F64) - ref[k]))) if ref[k].size else 0.0
        out[k] = (ref[k], np.full(ref[k].shape, b))
    if op == "gcn_pretrain" and case[6].startswith("saturated"):
        p0 = np.concatenate([inp[k].ravel() for k in ("w1", "b1", "w2", "b2")]).astype(F64)
        for k, v in (("params", p0), ("exp_avg", np.zeros_like(p0)), ("exp_avg_sq", np.zeros_like(p0))):
            out[k] = (v, np.zeros_like(p0))
    if op == "gcn_pretrain":
        del out["loss"]                                       # judged over the table: loss_table_bound
        out["_loss"] = (float(ref["loss"][0]), float(mir["loss"][0]))
    if op == "gnn":
        ub = BOUND_FACTOR * float(np.max(np.abs(mir["_U"].astype(F64) - ref["_U"])))
        out["_excluded"] = np.flatnonzero((np.abs(ref["_U"]) < ub).any(axis=0))
    return out


def excluded_fraction(case, refs) -> float:
    F, hid, od = case[2:5]
    return len(refs["_excluded"]) * (F + 1) / float(hid * F + hid + od * hid + od)


def figures(op, case, got: Dict[str, np.ndarray], refs) -> Dict[str, tuple]:
    """{output: (error, bound, error / bound)} at the element where error / bound is worst (the ratio is inf where a bit-exact
    output differs or a NaN came out)."""
    out = {}
    ex = refs.get("_excluded", ())
    for k in refs:
        if k.startswith("_"):
            continue
        ref, bound = refs[k]
        g = np.asarray(got[k], dtype=F64).reshape(ref.shape)
        if len(ex) and k in ("g_w1", "g_b1"):
            keep = np.setdiff1d(np.arange(ref.shape[0]), ex)
            g, ref, bound = g[keep], ref[keep], bound[keep]
        ratio = worst_ratio(g, ref, bound)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(np.isnan(g) | np.isnan(ref), np.inf, np.abs(g - ref))
            rel = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        at = np.unravel_index(int(np.argmax(rel)), rel.shape) if rel.size else ()
        out[k] = (float(err[at]), float(bound[at]), ratio) if rel.size else (0.0, 0.0, ratio)
    return out


def check(op, case, got: Dict[str, np.ndarray], refs) -> Dict[str, float]:
    """error / bound of every output."""
    return {k: v[2] for k, v in figures(op, case, got, refs).items()}


def loss_table_ratio(got_losses, refs_list) -> float:
    """The pretrain losses as ONE output over the table: max relative error of `got` over BOUND_FACTOR x the restatement's."""
    g = max(abs(float(x) - r["_loss"][0]) / abs(r["_loss"][0]) for x, r in zip(got_losses, refs_list))
    m = max(abs(r["_loss"][1] - r["_loss"][0]) / abs(r["_loss"][0]) for r in refs_list)
    if not all(math.isfinite(float(x)) for x in got_losses):
        return math.inf
    return g / (BOUND_FACTOR * m)


def outside_fraction(got, ref, bound) -> float:
    """The share of elements of `got` further than the bound from `ref` (the negative controls of the dropout sites)."""
    return float((np.abs(np.asarray(got, dtype=F64) - ref) > bound).mean())
