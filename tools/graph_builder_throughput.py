#!/usr/bin/env python3
"""Time per call of the graph builder (ultrafnd_git_amd/graph_builder.py) at N in {1000, 3600, 16384}, D = 416, k = 8:
cosine_knn_indices (the selection alone), cosine_knn (selection + the dense 0/1 graph) and build_dense_adj (selection + kNN
membership, OCR-overlap and delay weights in one pass over A).  Device events around windows of >= 0.5 s after warm-up, three
windows per measurement, alternated; the median is reported.  The host work of a call (phrase sets -> CSR, uploads) is inside
the window of the public functions and outside that of the two C entries, which are timed on device-resident operands too.

    graph_builder_throughput.py                          GPU timings (needs the MI355X; no fallback)
    graph_builder_throughput.py --reference DIR [N ...]  the reference's own CPU functions (DIR = its checkout; NumPy only),
                                                         one run per size on this host's CPU, no GPU involved

profiles/graph_builder_throughput.txt holds the output of both modes.
"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

SIZES, D, K = (1000, 3600, 16384), 416, 8


def inputs(n):
    """Standard-normal features, delay scores in [0, 1), and phrase sets with structure: a post draws 1..13 phrases from one of
    12 pools of 24 plus up to 4 stray ones out of a vocabulary of 400; about 6 % of the posts have no OCR text."""
    g = np.random.default_rng(n)
    pools = [g.choice(400, size=24, replace=False) for _ in range(12)]
    sets = []
    for _ in range(n):
        if g.random() < 0.06:
            sets.append(set())
            continue
        s = set(int(x) for x in g.choice(pools[g.integers(12)], size=g.integers(1, 14), replace=False))
        sets.append(s | set(int(x) for x in g.integers(0, 400, size=g.integers(0, 5))))
    return g.standard_normal((n, D)).astype(np.float32), sets, g.random(n).astype(np.float32)


def reference_cpu(ref_dir, sizes):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_dir)
    from src.models.gnn import graph_builder as R
    print(f"# the reference's src/models/gnn/graph_builder.py on this host's CPU (NumPy {np.__version__}), one run per size, wall clock")
    for n in sizes:
        X, sets, delay = inputs(n)
        t0 = time.perf_counter()
        A = R.cosine_knn(X, k=K)
        t1 = time.perf_counter()
        A = R.add_ocr_overlap_weights(A, sets)
        t2 = time.perf_counter()
        R.add_temporal_inconsistency(A, delay)
        t3 = time.perf_counter()
        print(f"reference CPU N={n}: cosine_knn {t1 - t0:.2f} s, add_ocr_overlap_weights {t2 - t1:.2f} s, "
              f"add_temporal_inconsistency {t3 - t2:.2f} s, build_dense_adj (the three) {t3 - t0:.2f} s", flush=True)


if len(sys.argv) > 2 and sys.argv[1] == "--reference":
    reference_cpu(sys.argv[2], [int(a) for a in sys.argv[3:]] or SIZES)
    sys.exit(0)

import torch

from ultrafnd_git_amd import _lib as L
from ultrafnd_git_amd import graph_builder as GB

if not torch.cuda.is_available():
    raise SystemExit("graph_builder_throughput.py: no HIP device (timings are taken on the GPU only)")
DEV = torch.device("cuda")


def timed(fn, window_s=0.5):
    """ms per call over a window of at least `window_s` seconds (device events around the whole window)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(3, int(window_s / max(time.perf_counter() - t0, 1e-5)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


print(f"# tools/graph_builder_throughput.py on one MI355X: D = {D}, k = {K}; device events over windows of >= 0.5 s after warm-up, three "
      "windows per path (alternated), median")
for n in SIZES:
    X, sets, delay = inputs(n)
    Xd, dd = torch.from_numpy(X).to(DEV), torch.from_numpy(delay).to(DEV)
    csr = GB._csr(sets, n, DEV)
    ws = torch.empty(L.lib().ufnd_cosine_knn_workspace_floats(n, D, K), dtype=torch.float32, device=DEV)
    idx = torch.empty(n, K, dtype=torch.int32, device=DEV)
    adj = torch.empty(n, n, dtype=torch.float32, device=DEV)
    s = L.stream_ptr(DEV)

    def entry_knn():
        L.check(L.lib().ufnd_cosine_knn(Xd.data_ptr(), D, n, D, K, idx.data_ptr(), ws.data_ptr(), s), "ufnd_cosine_knn")

    def entry_adj():
        L.check(L.lib().ufnd_dense_adj(idx.data_ptr(), K, csr[0].data_ptr(), csr[1].data_ptr(), dd.data_ptr(), 0.4, 0.25, n,
                                       adj.data_ptr(), n, L.ADJ_KNN | L.ADJ_OCR | L.ADJ_TEMPORAL, s), "ufnd_dense_adj")

    paths = (("ufnd_cosine_knn (entry, device operands)", entry_knn),
             ("ufnd_dense_adj KNN|OCR|TEMPORAL (entry, device operands)", entry_adj),
             ("cosine_knn_indices(X)", lambda: GB.cosine_knn_indices(Xd, K)),
             ("cosine_knn(X)", lambda: GB.cosine_knn(Xd, K)),
             ("build_dense_adj(X, sets, delay) incl. sets -> CSR on the host", lambda: GB.build_dense_adj(Xd, sets, dd, K)))
    res = {name: [] for name, _ in paths}
    for rnd in range(3):
        for name, fn in paths:
            res[name].append(timed(fn))
    flops = 2.0 * n * n * D
    for name, _ in paths:
        ms = [m for m, _ in res[name]]
        med = statistics.median(ms)
        extra = f"; S = Xn Xn^T alone is {flops / 1e9:.1f} GFLOP -> {flops / (med * 1e-3) / 1e12:.2f} TFLOP/s of the whole call" \
            if name.startswith("ufnd_cosine_knn") else ""
        print(f"N={n}: {name}: {med:.3f} ms per call (three windows: {', '.join(f'{m:.3f}' for m in ms)}; "
              f"{res[name][0][1]} calls per window){extra}", flush=True)
