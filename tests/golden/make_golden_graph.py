"""Mints tests/golden/graph_builder.npz from the REAL reference graph builder (src/models/gnn/graph_builder.py; the import needs
NumPy only), the way make_golden_explain.py mints explain.npz.  Run from the repository root; the reference checkout is
taken from $UFND_REFERENCE, by default the directory `reference` beside the repository:

    python tests/golden/make_golden_graph.py

N = 300, D = 416, k = 8.  X and the phrase sets are regenerated from their seeds (tests/graph_builder_ref.py: features,
ocr_sets); stored are the seeds, the delay scores (float32), the reference's kNN graph bit-packed as in gcn.npz, and the
nonzeros -- flat indices plus values -- of three weighted graphs, all from the reference's own functions:
    ocr       add_ocr_overlap_weights(kNN graph)
    temporal  add_temporal_inconsistency(kNN graph)            (its nonzeros are the kNN graph's)
    full      build_dense_adj(X, sets, delay)                  (same nonzeros as ocr)
Before it writes, the script asserts that the restatement's two weightings reproduce the reference's bit for bit, that the
reference's kNN graph lies inside the restatement's bounds, and that the share of ambiguous rows of every test input is
under the cap.  No test reads the reference.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
REF = Path(os.environ.get("UFND_REFERENCE", REPO.parent / "reference"))      # the reference checkout
sys.path.insert(0, str(REPO))


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    from src.models.gnn import graph_builder as R
    from tests import graph_builder_ref as G

    f = G.FIXTURE
    n, d, k = f["N"], f["D"], f["k"]
    X, sets = G.fixture_inputs()
    delay = G.delay_scores(n, f["delay_seed"])
    assert delay.dtype == np.float32

    knn = R.cosine_knn(X, k=k)
    S, t = G.similarity64(X), G.tau(d)
    lo, hi = G.bounds(S, k, t)
    G.check_adj(knn, lo, hi)
    print(f"reference kNN graph inside the bounds; {int((lo != hi).sum())} undetermined entries, "
          f"{G.ambiguous_rows(S, k, t)} ambiguous rows of {n}")

    ocr = R.add_ocr_overlap_weights(knn.copy(), sets, alpha=f["alpha"])
    tmp = R.add_temporal_inconsistency(knn.copy(), delay, beta=f["beta"])
    full = R.build_dense_adj(X, sets, delay, k=k, alpha=f["alpha"], beta=f["beta"])
    for a in (knn, ocr, tmp, full):
        assert a.dtype == np.float32 and np.array_equal(a, a.T)
    assert np.array_equal(G.add_ocr_overlap_weights(knn, sets, f["alpha"]), ocr), "OCR restatement"
    assert np.array_equal(G.add_temporal_inconsistency(knn, delay, f["beta"]), tmp), "temporal restatement"
    assert np.array_equal(G.weighted(knn, sets, delay, f["alpha"], f["beta"]), full), "build_dense_adj restatement"
    assert np.array_equal(tmp != 0, knn != 0) and np.array_equal(full != 0, ocr != 0)
    print("restatement reproduces the reference's weights exactly")

    for (n_, d_, k_, seed_) in G.INPUTS:
        X_ = G.features(n_, d_, seed_)
        S_ = G.similarity64(X_)
        amb = G.ambiguous_rows(S_, k_, G.tau(d_))
        lo_, hi_ = G.bounds(S_, k_, G.tau(d_))
        G.check_adj(R.cosine_knn(X_, k=k_), lo_, hi_)
        print(f"N={n_} D={d_} k={k_} seed={seed_}: {amb} ambiguous rows ({100.0 * amb / n_:.1f} %), reference inside the bounds")
        assert amb <= G.AMBIGUOUS_CAP * n_

    nz = np.flatnonzero(ocr).astype(np.int32)
    store = {"N": np.int64(n), "D": np.int64(d), "k": np.int64(k), "seed": np.int64(f["seed"]), "set_seed": np.int64(f["set_seed"]),
             "delay_seed": np.int64(f["delay_seed"]), "alpha": np.float64(f["alpha"]), "beta": np.float64(f["beta"]), "delay": delay,
             "knn_packed": np.packbits(knn.astype(np.uint8), axis=1), "nz_index": nz, "ocr_values": ocr.reshape(-1)[nz],
             "full_values": full.reshape(-1)[nz], "temporal_values": tmp.reshape(-1)[np.flatnonzero(knn)],
             "x_checksum": np.float64(X.astype(np.float64).sum())}
    out = HERE / "graph_builder.npz"
    np.savez_compressed(out, **store)
    print(out, out.stat().st_size, "bytes")
    assert out.stat().st_size < 200 * 1024


if __name__ == "__main__":
    main()
