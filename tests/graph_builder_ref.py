"""Our own vectorised NumPy restatement of the reference's graph builder (src/models/gnn/graph_builder.py) and the
structural bounds a kNN result is held to.  Not the reference's loops; tests/golden/make_golden_graph.py asserts, before it
mints tests/golden/graph_builder.npz, that the two weightings here reproduce the reference's exactly and that the
reference's own kNN graph lies inside the bounds.  No test reads the reference.

The selection.  The reference picks row i's neighbours from a float32 S with np.argpartition, so a near-tie between the
k-th and the (k+1)-th similarity is legitimately open.  S is computed here in float64 and
    tau = (4 D + 16) 2^-24
is the worst-case fp32 error of two compared dot products of fp32-normalised rows (the sum of squares and the dot product
each contribute at most D 2^-24 per product).  With s_k(i) the k-th largest S[i][j], j != i:
    j is CERTAIN  for row i if S_ij >  s_k(i) + tau,
    j is POSSIBLE for row i if S_ij >= s_k(i) - tau,
A_lo / A_hi are the symmetrised graphs (unit diagonal) of the certain / possible sets.  A kNN result is valid when every row
of idx holds exactly k distinct indices, none equal to i, all certain ones present and none outside the possible set, and
A_lo <= A <= A_hi elementwise.  A row is AMBIGUOUS if s_k - s_{k+1} < tau; at most 10 % of the rows of a test input may be.

The weightings, in the NumPy dtypes the reference's statements produce on a float32 A:
    OCR       A[i][j] += alpha * np.log1p(ov)            float32 + float64 -> float64, stored as float32
    temporal  A[i][j] *= 1.0 + beta * abs(d_i - d_j)     float32 delay scores: every operation in float32
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

# (N, D, k, seed): X = default_rng(seed).standard_normal((N, D)) as float32.  Ambiguous rows (float64 gap below tau):
# 0, 0, 0, 0, 13, 43 (8.4 %), 52.
INPUTS = [(10, 416, 8, 1), (67, 416, 8, 2), (130, 20, 8, 3), (257, 5, 3, 5), (300, 416, 8, 4), (513, 416, 16, 7), (1000, 416, 8, 6)]
AMBIGUOUS_CAP = 0.10
WEIGHT_RTOL = 4.0 * 2.0 ** -24     # three fp32 roundings that may differ + a double log1p that may differ in its last bit
FIXTURE = dict(N=300, D=416, k=8, seed=4, set_seed=11, delay_seed=12, alpha=0.4, beta=0.25)


def features(n: int, d: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def delay_scores(n: int, seed: int) -> np.ndarray:
    """[N] float32 in [0, 1) (the reference's docstring: lip-sync lag scores in [0, 1])."""
    return np.random.default_rng(seed).random(n).astype(np.float32)


def ocr_sets(n: int, seed: int) -> List[set]:
    from oracle.gcn_ref import synthetic_ocr_sets
    return synthetic_ocr_sets(n, seed)


def tau(d: int) -> float:
    return (4.0 * d + 16.0) * 2.0 ** -24


def similarity64(X: np.ndarray) -> np.ndarray:
    """S = Xn Xn^T in float64 from the float32 X, -inf on the diagonal."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    Xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + 1e-9)
    S = Xn @ Xn.T
    np.fill_diagonal(S, -np.inf)
    return S


def _kth(S: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """(s_k, s_{k+1}) of every row; s_{k+1} = -inf when a row has only k candidates."""
    srt = -np.sort(-S, axis=1)
    return srt[:, k - 1], (srt[:, k] if k < S.shape[1] - 1 else np.full(S.shape[0], -np.inf))


def ambiguous_rows(S: np.ndarray, k: int, t: float) -> int:
    sk, sk1 = _kth(S, k)
    return int(np.count_nonzero(sk - sk1 < t))


def candidate_sets(S: np.ndarray, k: int, t: float) -> Tuple[np.ndarray, np.ndarray]:
    """(certain, possible) boolean (N, N); the diagonal is in neither."""
    sk = _kth(S, k)[0][:, None]
    return S > sk + t, S >= sk - t


def _symmetrised(m: np.ndarray) -> np.ndarray:
    a = (m | m.T).astype(np.float32)
    np.fill_diagonal(a, 1.0)
    return a


def bounds(S: np.ndarray, k: int, t: float) -> Tuple[np.ndarray, np.ndarray]:
    """(A_lo, A_hi) float32."""
    certain, possible = candidate_sets(S, k, t)
    return _symmetrised(certain), _symmetrised(possible)


def adj_from_indices(idx: np.ndarray, n: int) -> np.ndarray:
    m = np.zeros((n, n), dtype=bool)
    m[np.repeat(np.arange(n), idx.shape[1]), idx.reshape(-1)] = True
    return _symmetrised(m)


def check_indices(idx: np.ndarray, S: np.ndarray, k: int, t: float) -> None:
    """Every row: k distinct indices in range, none equal to i, all certain ones present, none outside the possible set."""
    n = S.shape[0]
    idx = np.asarray(idx)
    assert idx.shape == (n, k), (idx.shape, n, k)
    assert idx.min() >= 0 and idx.max() < n
    rows = np.arange(n)[:, None]
    assert not (idx == rows).any(), "a row lists itself"
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a row lists an index twice"
    certain, possible = candidate_sets(S, k, t)
    chosen = np.zeros((n, n), dtype=bool)
    chosen[np.repeat(np.arange(n), k), idx.reshape(-1)] = True
    bad = np.flatnonzero((certain & ~chosen).any(1) | (chosen & ~possible).any(1))
    assert bad.size == 0, f"rows {bad[:8].tolist()} miss a certain neighbour or hold an impossible one"


def check_adj(A: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> None:
    A = np.asarray(A)
    assert A.shape == lo.shape and np.isin(A, (0.0, 1.0)).all()
    assert (lo <= A).all() and (A <= hi).all(), "A outside [A_lo, A_hi]"


def check_order(idx: np.ndarray, S: np.ndarray, t: float) -> None:
    """Rows are listed by similarity descending, up to the fp32 rounding of two compared similarities."""
    v = np.take_along_axis(S, np.asarray(idx, dtype=np.int64), axis=1)
    assert (v[:, :-1] >= v[:, 1:] - t).all()


def overlap_counts(sets: Sequence[set]) -> np.ndarray:
    """(N, N) int64 |set_i & set_j| through the incidence matrix."""
    vocab = {}
    rows, cols = [], []
    for i, s in enumerate(sets):
        for ph in s:
            rows.append(i)
            cols.append(vocab.setdefault(ph, len(vocab)))
    M = np.zeros((len(sets), max(1, len(vocab))), dtype=np.int64)
    M[rows, cols] = 1
    return M @ M.T


def add_ocr_overlap_weights(A: np.ndarray, sets: Sequence[set], alpha: float = 0.4) -> np.ndarray:
    """A new float32 array (the reference mutates its argument)."""
    A = np.asarray(A, dtype=np.float32)
    ov = overlap_counts(sets)
    np.fill_diagonal(ov, 0)
    w = alpha * np.log1p(ov.astype(np.float64))                     # float64, 0 where the sets do not meet
    return np.where(ov > 0, (A.astype(np.float64) + w).astype(np.float32), A)


def add_temporal_inconsistency(A: np.ndarray, delay: np.ndarray, beta: float = 0.25) -> np.ndarray:
    A = np.asarray(A, dtype=np.float32)
    d = np.asarray(delay, dtype=np.float32)
    w = np.float32(1.0) + np.float32(beta) * np.abs(d[:, None] - d[None, :])      # float32 throughout
    assert w.dtype == np.float32
    out = A * w
    np.fill_diagonal(out, np.diagonal(A))
    return out


def weighted(A: np.ndarray, sets: Sequence[set], delay: np.ndarray, alpha: float = 0.4, beta: float = 0.25) -> np.ndarray:
    """build_dense_adj after its kNN step."""
    return add_temporal_inconsistency(add_ocr_overlap_weights(A, sets, alpha), delay, beta)


def max_rel_err(got: np.ndarray, ref: np.ndarray, where: np.ndarray) -> float:
    g, r = np.asarray(got, dtype=np.float64)[where], np.asarray(ref, dtype=np.float64)[where]
    assert np.array_equal(g == 0, r == 0), "the two disagree on which entries are zero"
    nz = r != 0
    return float((np.abs(g[nz] - r[nz]) / np.abs(r[nz])).max()) if nz.any() else 0.0


# ---- the fixture (tests/golden/graph_builder.npz)
def fixture_inputs():
    f = FIXTURE
    return features(f["N"], f["D"], f["seed"]), ocr_sets(f["N"], f["set_seed"])


def unpack_fixture(z) -> dict:
    n = int(z["N"])
    knn = np.unpackbits(z["knn_packed"], axis=1)[:, :n].astype(np.float32)
    out = {"knn": knn, "delay": z["delay"]}
    for name in ("ocr", "full"):
        a = np.zeros(n * n, dtype=np.float32)
        a[z["nz_index"]] = z[f"{name}_values"]
        out[name] = a.reshape(n, n)
    t = np.zeros(n * n, dtype=np.float32)
    t[np.flatnonzero(knn)] = z["temporal_values"]
    out["temporal"] = t.reshape(n, n)
    return out
