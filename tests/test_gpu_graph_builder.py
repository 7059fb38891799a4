"""GPU checks of the graph builder (ultrafnd_git_amd/graph_builder.py over ufnd_cosine_knn / ufnd_dense_adj) against the
fixture minted from the real reference (tests/golden/graph_builder.npz) and the bounds and weightings of
tests/graph_builder_ref.py.  Criteria (see that module): a kNN result must be valid row by row and lie in [A_lo, A_hi];
weights agree with the reference within 4 * 2^-24 relative wherever the graph is determined; the fp32 temporal factor on a
0/1 graph is bit-exact."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import graph_builder_ref as G
from tests.helpers import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"

# beyond the table: all others are neighbours (N = 9, k = 8); k = 1 and k = 64 (D = 33: no multiple of the 32-wide staging chunk)
EXTRA = [(9, 416, 8, 8), (200, 33, 1, 9), (200, 33, 64, 10)]


@functools.lru_cache(maxsize=None)
def _case(n, d, k, seed):
    X = G.features(n, d, seed)
    S, t = G.similarity64(X), G.tau(d)
    assert G.ambiguous_rows(S, k, t) <= G.AMBIGUOUS_CAP * n
    return X, S, t, G.bounds(S, k, t)


@functools.lru_cache(maxsize=None)
def _fixture():
    z = load_npz("graph_builder.npz")
    X, sets = G.fixture_inputs()
    assert float(X.astype(np.float64).sum()) == float(z["x_checksum"])
    return X, sets, G.unpack_fixture(z)


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_fixture():
    from ultrafnd_git_amd import graph_builder as GB
    X, sets, fx = _fixture()
    f = G.FIXTURE
    n, k, a, b = f["N"], f["k"], f["alpha"], f["beta"]
    _, S, t, (lo, hi) = _case(n, f["D"], k, f["seed"])
    det = lo == hi
    # kNN graph: inside the bounds, and equal to the reference's wherever the graph is determined
    A = _np(GB.cosine_knn(X, k))
    G.check_adj(A, lo, hi)
    assert np.array_equal(A, A.T)
    assert np.array_equal(A[det], fx["knn"][det])
    print(f"fixture: {int((~det).sum())} undetermined entries; ours differs from the reference's kNN graph on {int((A != fx['knn']).sum())}")
    # each weighting alone, on the reference's kNN graph; both mutate their argument and return it
    T = _dev(fx["knn"])
    out = GB.add_temporal_inconsistency(T, fx["delay"], b)
    assert out is T
    assert np.array_equal(_np(T), fx["temporal"]), "the fp32 temporal factor on a 0/1 graph must be bit-exact"
    O = _dev(fx["knn"])
    assert GB.add_ocr_overlap_weights(O, [set(f"phrase{p}" for p in s) for s in sets], a) is O       # phrases as strings, like the reference
    e_ocr = G.max_rel_err(_np(O), fx["ocr"], np.ones_like(det))
    # build_dense_adj: against the fixture where determined, against the restatement on our own kNN graph everywhere
    full = _np(GB.build_dense_adj(X, sets, fx["delay"], k, a, b))
    assert np.array_equal(full != 0, G.weighted(A, sets, fx["delay"], a, b) != 0)
    e_fix = G.max_rel_err(full, fx["full"], det)
    e_ref = G.max_rel_err(full, G.weighted(A, sets, fx["delay"], a, b), np.ones_like(det))
    print(f"max relative error: OCR alone {e_ocr:.3e}, build_dense_adj vs fixture {e_fix:.3e}, vs restatement {e_ref:.3e} "
          f"(bound {G.WEIGHT_RTOL:.3e})")
    assert max(e_ocr, e_fix, e_ref) <= G.WEIGHT_RTOL
    assert np.array_equal(full, full.T) and (np.diagonal(full) == 1).all()


@pytest.mark.parametrize("n,d,k,seed", G.INPUTS + EXTRA)
def test_knn_bounds_and_consistency(n, d, k, seed):
    from ultrafnd_git_amd import graph_builder as GB
    X, S, t, (lo, hi) = _case(n, d, k, seed)
    Xd = _dev(X)
    idx = GB.cosine_knn_indices(Xd, k)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (n, k) and idx.device.type == "cuda"
    G.check_indices(_np(idx), S, k, t)
    G.check_order(_np(idx), S, t)
    A = GB.cosine_knn(Xd, k)
    assert A.dtype == torch.float32 and tuple(A.shape) == (n, n)
    G.check_adj(_np(A), lo, hi)
    assert np.array_equal(_np(A), G.adj_from_indices(_np(idx), n)), "the dense graph is the symmetrised index lists"
    # no atomics, no order dependence: a second run (from a NumPy input this time) gives the same bits
    assert torch.equal(GB.cosine_knn_indices(X, k), idx) and torch.equal(GB.cosine_knn(X, k), A)
    if n == 9:
        assert np.array_equal(_np(A), np.ones((9, 9), dtype=np.float32))


def test_strided_input_is_read_in_place():
    from ultrafnd_git_amd import graph_builder as GB
    n, d, k, seed = G.INPUTS[2]
    X, S, t, _ = _case(n, d, k, seed)
    wide = torch.full((n, d + 7), 1e3, device=DEV)
    wide[:, :d] = _dev(X)
    view = wide[:, :d]
    assert view.stride(0) == d + 7 and GB._features(view, view.device).data_ptr() == wide.data_ptr()
    idx = GB.cosine_knn_indices(view, k)
    G.check_indices(_np(idx), S, k, t)
    assert torch.equal(idx, GB.cosine_knn_indices(_dev(X), k))


def test_exact_ties_go_to_the_lower_index():
    from ultrafnd_git_amd import graph_builder as GB
    # (inputs made of exact ties: every row is ambiguous by construction, so only validity and the tie rule are checked)
    # every row twice (rows 2m and 2m + 1 are equal): a row's list is its twin, then whole pairs, each exactly tied; with k = 4
    # the list ends in the middle of a pair, which must be the pair's even member
    base = G.features(40, 24, 21)
    X = np.repeat(base, 2, axis=0)
    n, k = X.shape[0], 4
    S, t = G.similarity64(X), G.tau(24)
    idx = _np(GB.cosine_knn_indices(X, k))
    G.check_indices(idx, S, k, t)
    rows = np.arange(n)
    assert np.array_equal(idx[:, 0], rows ^ 1), "the nearest row is the twin"
    assert (idx[:, 1] % 2 == 0).all() and np.array_equal(idx[:, 2], idx[:, 1] + 1) and (idx[:, 3] % 2 == 0).all()
    G.check_adj(_np(GB.cosine_knn(X, k)), *G.bounds(S, k, t))
    # one duplicated pair among distinct rows: wherever the later twin is listed, the earlier one stands right before it
    n, d, k, seed = G.INPUTS[1]
    X = G.features(n, d, seed).copy()
    X[41] = X[17]
    S, t = G.similarity64(X), G.tau(d)
    idx = _np(GB.cosine_knn_indices(X, k))
    G.check_indices(idx, S, k, t)
    assert idx[17, 0] == 41 and idx[41, 0] == 17
    for i in range(n):
        pos = np.flatnonzero(idx[i] == 41)
        if i not in (17, 41) and pos.size:
            assert pos[0] >= 1 and idx[i, pos[0] - 1] == 17, i


def test_all_zero_row():
    from ultrafnd_git_amd import graph_builder as GB
    n, d, k, seed = G.INPUTS[1]
    X = G.features(n, d, seed).copy()
    X[5] = 0.0
    S, t = G.similarity64(X), G.tau(d)
    idx = _np(GB.cosine_knn_indices(X, k))
    G.check_indices(idx, S, k, t)
    assert idx[5].tolist() == [0, 1, 2, 3, 4, 6, 7, 8]      # every similarity of the row is exactly 0: the lowest indices
    A = _np(GB.cosine_knn(X, k))
    G.check_adj(A, *G.bounds(S, k, t))
    assert np.isfinite(A).all()


def test_build_dense_adj_equals_the_three_calls():
    from ultrafnd_git_amd import graph_builder as GB
    for (n, d, k, seed) in (G.INPUTS[2], G.INPUTS[4]):
        X, sets, delay = G.features(n, d, seed), G.ocr_sets(n, seed + 100), G.delay_scores(n, seed + 200)
        one = GB.build_dense_adj(X, sets, delay, k, 0.3, 0.7)
        A = GB.cosine_knn(X, k)
        knn = A.clone()
        A = GB.add_temporal_inconsistency(GB.add_ocr_overlap_weights(A, sets, 0.3), delay, 0.7)
        assert torch.equal(one, A) and not torch.equal(A, knn)
        ref = G.weighted(_np(knn), sets, delay, 0.3, 0.7)
        e = G.max_rel_err(_np(one), ref, np.ones((n, n), dtype=bool))
        print(f"N={n}: build_dense_adj vs restatement on its own kNN graph, max relative error {e:.3e}")
        assert e <= G.WEIGHT_RTOL
    # delay scores given in float64 are rounded to fp32 on entry
    assert torch.equal(GB.build_dense_adj(X, sets, delay.astype(np.float64), k, 0.3, 0.7), one)


def test_weightings_edge_cases():
    """The OCR cases of tests/test_gpu_gcn.py: sets longer than the kernel's LDS window, empty sets, a single node."""
    from ultrafnd_git_amd import graph_builder as GB
    g = np.random.default_rng(5)
    big = [set(range(0, 5000)), set(range(2500, 7500)), set(range(100000, 100010)), set(), set(range(4990, 5010))]
    A0 = (g.random((5, 5)) * 2).astype(np.float32)           # weighted, asymmetric, non-unit diagonal: an arbitrary A is updated
    got = _np(GB.add_ocr_overlap_weights(_dev(A0), big, 0.4))
    ref = G.add_ocr_overlap_weights(A0, big, 0.4)
    e = G.max_rel_err(got, ref, np.ones((5, 5), dtype=bool))
    print(f"long sets: max relative error {e:.3e}")
    assert e <= G.WEIGHT_RTOL and np.array_equal(np.diagonal(got), np.diagonal(A0)) and got[0, 1] > A0[0, 1] + 3.0
    assert np.array_equal(got[3], A0[3]) and np.array_equal(got[:, 3], A0[:, 3])          # the empty set meets nothing
    # all sets empty: nothing changes, bit for bit
    assert np.array_equal(_np(GB.add_ocr_overlap_weights(_dev(A0), [set()] * 5, 0.4)), A0)
    # temporal on an arbitrary A: op by op in fp32 = the restatement's bits; zero delays leave A alone
    d = g.random(5).astype(np.float32)
    assert np.array_equal(_np(GB.add_temporal_inconsistency(_dev(A0), d, 0.25)), G.add_temporal_inconsistency(A0, d, 0.25))
    assert np.array_equal(_np(GB.add_temporal_inconsistency(_dev(A0), np.zeros(5), 0.25)), A0)
    # (beta = 0.25 makes fl(beta x) exact; at 0.7 and 1/3 a fused 1 + beta x would round differently)
    for beta in (0.7, 1.0 / 3.0):
        assert np.array_equal(_np(GB.add_temporal_inconsistency(_dev(A0), d, beta)), G.add_temporal_inconsistency(A0, d, beta)), beta
    many, dm = G.ocr_sets(700, 9), G.delay_scores(700, 10)
    Am = (g.random((700, 700)) < 0.05).astype(np.float32)
    for beta in (0.25, 0.7):
        assert np.array_equal(_np(GB.add_temporal_inconsistency(_dev(Am), dm, beta)), G.add_temporal_inconsistency(Am, dm, beta)), beta
    e = G.max_rel_err(_np(GB.add_ocr_overlap_weights(_dev(Am), many, 0.4)), G.add_ocr_overlap_weights(Am, many, 0.4),
                      np.ones((700, 700), dtype=bool))
    print(f"N=700: OCR max relative error {e:.3e}")
    assert e <= G.WEIGHT_RTOL
    # N = 1: the only entry is the diagonal, which is never weighted
    one = torch.full((1, 1), 1.0, device=DEV)
    assert GB.add_ocr_overlap_weights(one, [{1, 2}], 0.4).item() == 1.0
    assert GB.add_temporal_inconsistency(one, np.array([0.7]), 0.25).item() == 1.0
    # a row-strided A is updated in place
    wide = torch.zeros(5, 9, device=DEV)
    wide[:, :5] = _dev(A0)
    GB.add_temporal_inconsistency(wide[:, :5], d, 0.25)
    assert np.array_equal(_np(wide[:, :5]), G.add_temporal_inconsistency(A0, d, 0.25)) and (wide[:, 5:] == 0).all()


def test_c_abi_refusals_by_name():
    from ultrafnd_git_amd import _lib as L
    lib = L.lib()
    X = torch.randn(20, 16, device=DEV)
    idx = torch.zeros(20, 64, dtype=torch.int32, device=DEV)
    assert lib.ufnd_cosine_knn_workspace_floats(20, 16, 4) == 20 * 32 and lib.ufnd_cosine_knn_workspace_floats(20, 33, 4) == 20 * 64
    assert lib.ufnd_cosine_knn_workspace_floats(0, 16, 4) == 0
    ws = torch.empty(20 * 32, device=DEV)
    s = L.stream_ptr(X.device)

    def knn(n, d, k, ldx=16):
        rc = lib.ufnd_cosine_knn(X.data_ptr(), ldx, n, d, k, idx.data_ptr(), ws.data_ptr(), s)
        return rc, lib.ufnd_last_error().decode()

    for args, word in (((20, 16, 0), "k=0"), ((20, 16, 65), "k=65"), ((20, 16, 20), "k < N"), ((20, 16, 4, 15), "ldx=15"), ((20, 0, 4), "D=0")):
        rc, msg = knn(*args)
        assert rc != 0 and word in msg, (args, msg)
    assert knn(20, 16, 4)[0] == 0
    adj = torch.zeros(20, 20, device=DEV)
    for flags, k, word in ((0, 4, "flags"), (8, 4, "flags"), (L.ADJ_KNN, 65, "k=65"), (L.ADJ_KNN, 20, "k < N"), (L.ADJ_OCR, 4, "offsets"),
                           (L.ADJ_TEMPORAL, 4, "delay")):
        rc = lib.ufnd_dense_adj(idx.data_ptr(), k, None, None, None, 0.4, 0.25, 20, adj.data_ptr(), 20, flags, s)
        assert rc != 0 and word in lib.ufnd_last_error().decode(), (flags, k, lib.ufnd_last_error().decode())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ trainer
def _cache(n, seed, with_sets=True, with_delay=True):
    from ultrafnd_git_amd.trainer import synthetic_cache
    cache = synthetic_cache(n, seed=seed)
    del cache["gnn_Z"]
    if with_sets:
        cache["ocr_sets"] = G.ocr_sets(n, seed + 1)
    if with_delay:
        cache["delay_scores"] = G.delay_scores(n, seed + 2)
    return cache


def test_trainer_default_graph_is_unchanged(tmp_path):
    """gnn_graph defaults to "ocr": Adj and gnn_Z are, bit for bit, what the construction spelled out step by step gives."""
    from oracle import gcn_ref
    from ultrafnd_git_amd import gcn
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig
    cache = _cache(96, 3)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=16, epochs=1, device=DEV, seed=7)
    tr = ForensicTrainer(cfg, cache=cache)
    assert np.array_equal(_np(tr.Adj), gcn_ref.build_adj_from_ocr(cache["ocr_sets"], 0.12))
    torch.manual_seed(7)
    np.random.seed(7)
    X = torch.from_numpy(gcn.node_features(cache)).to(DEV)
    Adj = gcn.build_adj_from_ocr(cache["ocr_sets"], 0.12, DEV)
    net = gcn.SimpleGCN(in_dim=416, hid=256, out_dim=128, dropout=0.2).to(DEV)
    gcn.pretrain_gnn(net, X, Adj, 128, epochs=2)
    Z = net(X, Adj)
    assert torch.equal(tr.Adj, Adj) and torch.equal(tr.cache["gnn_Z"], Z)
    tr2 = ForensicTrainer(TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=16, epochs=1, device=DEV,
                                      seed=7, gnn_graph="ocr", gnn_knn_k=3), cache=cache)
    assert torch.equal(tr2.Adj, Adj) and torch.equal(tr2.cache["gnn_Z"], Z)


def test_trainer_knn_graph(tmp_path):
    from ultrafnd_git_amd import gcn, graph_builder as GB
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig
    cache = _cache(96, 3)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=16, epochs=1, device=DEV, seed=7,
                      gnn_graph="knn", gnn_knn_k=5)
    tr = ForensicTrainer(cfg, cache=cache)
    Xn = gcn.node_features(cache)
    want = GB.build_dense_adj(Xn, cache["ocr_sets"], cache["delay_scores"], k=5)
    assert torch.equal(tr.Adj, want)
    # ... which is the restatement's weighting of a valid kNN graph of the node features
    S, t = G.similarity64(Xn), G.tau(Xn.shape[1])
    assert G.ambiguous_rows(S, 5, t) <= G.AMBIGUOUS_CAP * 96
    knn = _np(GB.cosine_knn(Xn, 5))
    G.check_adj(knn, *G.bounds(S, 5, t))
    assert (knn.sum(1) - 1 >= 5).all(), "every post has its k neighbours"
    e = G.max_rel_err(_np(tr.Adj), G.weighted(knn, cache["ocr_sets"], cache["delay_scores"]), np.ones((96, 96), dtype=bool))
    assert e <= G.WEIGHT_RTOL, e
    Z = tr.cache["gnn_Z"]
    assert tuple(Z.shape) == (96, 128) and torch.isfinite(Z).all() and tr.gnn is not None
    tr.fit()
    st = tr._checkpoint_state()
    assert st["cfg"]["gnn_graph"] == "knn" and st["cfg"]["gnn_knn_k"] == 5
    if os.path.exists(tr.ckpt_path):
        saved = torch.load(tr.ckpt_path, map_location="cpu", weights_only=False)["cfg"]
        assert saved["gnn_graph"] == "knn" and saved["gnn_knn_k"] == 5


def test_trainer_knn_graph_without_sets_or_delays(tmp_path):
    """A cache with neither gnn_Z nor ocr_sets builds its graph (the "ocr" graph cannot: KeyError)."""
    from ultrafnd_git_amd import gcn, graph_builder as GB
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig
    cache = _cache(64, 5, with_sets=False, with_delay=False)
    base = dict(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=16, epochs=1, device=DEV, seed=7)
    with pytest.raises(KeyError):
        ForensicTrainer(TrainConfig(**base), cache=cache)
    tr = ForensicTrainer(TrainConfig(**base, gnn_graph="knn"), cache=cache)
    # no sets, zero delays: the graph is the 0/1 kNN graph itself (a temporal factor of exactly 1)
    assert torch.equal(tr.Adj, GB.cosine_knn(gcn.node_features(cache), 8))
    assert torch.isfinite(tr.cache["gnn_Z"]).all()
    loss, metrics = tr._epoch_loop(tr.train_loader, "train")
    assert np.isfinite(loss) and "auc" in metrics
