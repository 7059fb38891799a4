"""GPU parity (through the C ABI) of the graph side of the trainer: OCR-Jaccard adjacency
(bit-exact), SimpleGCN forward and the degree pre-training steps against the fixture minted from the real
reference (tests/golden/gcn.npz) and against the oracle on other sizes."""
import numpy as np
import pytest
import torch

from oracle import gcn_ref as G
from tests.helpers import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fixture():
    z = load_npz("gcn.npz")
    n = int(z["N"])
    sets = G.synthetic_ocr_sets(n, int(z["set_seed"]))
    adj = np.unpackbits(z["adj_packed"], axis=1)[:, :n].astype(np.float32)
    return z, n, sets, adj


def test_ocr_adjacency_is_bit_exact():
    from ultrafnd_git_amd.gcn import build_adj_from_ocr
    z, n, sets, adj = _fixture()
    got = build_adj_from_ocr([set(f"phrase{t}" for t in s) for s in sets], 0.12, DEV).cpu().numpy()   # phrases as strings, like the reference
    assert np.array_equal(got, adj)
    for thr in (0.0, 0.05, 0.3, 1.0):
        assert np.array_equal(build_adj_from_ocr(sets, thr, DEV).cpu().numpy(), G.build_adj_from_ocr(sets, thr)), thr
    # ragged / edge cases: one node, all-empty sets, a set longer than the kernel's LDS window
    assert build_adj_from_ocr([set()], 0.12, DEV).cpu().numpy().tolist() == [[1.0]]
    e = build_adj_from_ocr([set(), set(), {1}], 0.12, DEV).cpu().numpy()
    assert np.array_equal(e, np.eye(3, dtype=np.float32))
    big = [set(range(0, 5000)), set(range(2500, 7500)), set(range(100000, 100010)), set()]
    assert np.array_equal(build_adj_from_ocr(big, 0.3, DEV).cpu().numpy(), G.build_adj_from_ocr(big, 0.3))
    g = np.random.RandomState(3)
    many = G.synthetic_ocr_sets(700, 9)
    assert np.array_equal(build_adj_from_ocr(many, 0.12, DEV).cpu().numpy(), G.build_adj_from_ocr(many, 0.12))


def _gcn(z):
    from ultrafnd_git_amd.gcn import SimpleGCN
    net = SimpleGCN(in_dim=416, hid=256, out_dim=128, dropout=0.2)
    net.load_state_dict(G.seeded_weights(int(z["weight_seed"])))
    return net.to(DEV)


def test_gcn_forward_matches_reference():
    z, n, sets, adj = _fixture()
    net = _gcn(z).eval()
    out = net(torch.from_numpy(z["X"]).to(DEV), torch.from_numpy(adj).to(DEV)).cpu()
    err = (out - torch.from_numpy(z["Z"])).abs().max().item()
    print(f"gcn forward max-abs-err vs reference {err:.2e} (|Z| max {np.abs(z['Z']).max():.2f})")
    assert err <= 2e-5
    assert list(net.state_dict().keys()) == ["lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"]


@pytest.mark.parametrize("n", [1, 33, 257])
def test_gcn_forward_other_sizes_vs_oracle(n):
    from ultrafnd_git_amd.gcn import SimpleGCN
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 64, generator=g)
    adj = (torch.rand(n, n, generator=g) < 0.1).float()
    adj = ((adj + adj.t()) > 0).float()
    adj.fill_diagonal_(1.0)
    w = G.seeded_weights(5, in_dim=64, hid=96, out_dim=32)
    net = SimpleGCN(64, 96, 32, dropout=0.3)
    net.load_state_dict(w)
    net = net.to(DEV).eval()
    out = net(x.to(DEV), adj.to(DEV)).cpu()
    assert (out - G.gcn_forward(w, x, adj)).abs().max().item() <= 2e-5


def test_pretrain_steps_match_reference_without_dropout():
    from ultrafnd_git_amd.gcn import pretrain_gnn
    import torch.nn as nn
    z, n, sets, adj = _fixture()
    net = _gcn(z)
    net.dropout = 0.0                  # the fixture's two Adam steps were run with p = 0 (RNG-free)
    head = nn.Linear(128, 1)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(z["head_w"])); head.bias.copy_(torch.from_numpy(z["head_b"]))
    X, A = torch.from_numpy(z["X"]).to(DEV), torch.from_numpy(adj).to(DEV)
    losses = pretrain_gnn(net, X, A, 128, epochs=2, head=head)
    assert np.abs(np.asarray(losses) - z["losses"]).max() <= 2e-6, (losses, z["losses"])
    sd = net.state_dict()
    assert abs(float(sd["lin1.weight"].double().sum()) - float(z["lin1_w_after_sum"])) <= 2e-3
    assert abs(float(sd["lin2.weight"].double().sum()) - float(z["lin2_w_after_sum"])) <= 2e-3
    w2, _ = G.pretrain(G.seeded_weights(int(z["weight_seed"])), torch.from_numpy(z["X"]), torch.from_numpy(adj),
                       torch.from_numpy(z["head_w"]), torch.from_numpy(z["head_b"]), epochs=2)
    for k in w2:       # Adam's first steps move every weight by ~lr: compare the UPDATE, not just the value
        upd_ref = (w2[k] - G.seeded_weights(int(z["weight_seed"]))[k])
        upd = sd[k].cpu() - G.seeded_weights(int(z["weight_seed"]))[k]
        assert (upd - upd_ref).abs().max().item() <= 2e-5 + 0.02 * upd_ref.abs().max().item(), k
    out = net.eval()(X, A).cpu()
    assert (out - torch.from_numpy(z["Z_after"])).abs().max().item() <= 1e-4


def test_train_mode_dropout_is_a_fresh_inverted_mask_per_call():
    z, n, sets, adj = _fixture()
    net = _gcn(z).train()
    X, A = torch.from_numpy(z["X"]).to(DEV), torch.from_numpy(adj).to(DEV)
    a, b = net(X, A), net(X, A)
    assert not torch.equal(a, b)
    ev = net.eval()(X, A)
    net.train()
    mean = torch.stack([net(X, A) for _ in range(64)]).mean(0)
    # inverted dropout is unbiased on the hidden layer; lin2 and A_norm are linear, so the mean approaches eval
    assert (mean - ev).abs().max().item() <= 0.25 * (a - ev).abs().max().item() + 1e-3


def test_trainer_builds_gnn_embeddings_from_ocr_sets():
    """ForensicTrainer._build_gnn (forensic_trainer.py:184-211): a cache WITHOUT gnn_Z but with ocr_sets."""
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    cache = synthetic_cache(96, seed=3)
    del cache["gnn_Z"]
    cache["ocr_sets"] = G.synthetic_ocr_sets(96, 4)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir="/tmp/ufnd_gcn_t", batch_size=16, epochs=1, device=DEV, seed=7)
    tr = ForensicTrainer(cfg, cache=cache)
    Z = tr.cache["gnn_Z"]
    assert tuple(Z.shape) == (96, 128) and torch.isfinite(Z).all() and tr.gnn is not None
    assert np.array_equal(tr.Adj.cpu().numpy(), G.build_adj_from_ocr(cache["ocr_sets"], 0.12))
    assert np.abs(tr.X.cpu().numpy() - G.node_features(cache["text"], cache["audio"], cache["visual"], cache["temporal"])).max() <= 1e-7
    loss, metrics = tr._epoch_loop(tr.train_loader, "train")
    assert np.isfinite(loss) and "auc" in metrics


@pytest.mark.parametrize("n_nodes", [None, 33])
def test_train_mode_steps_and_forward_match_the_oracle_run_with_the_mirrors_masks(n_nodes):
    """SimpleGCN's real setting (p = 0.2): two pre-training steps, then a train-mode forward, against the oracle given the masks
    the kernels should have drawn -- tag 9 (gcn.hip: LAYER_GCN), element row * hid + col, key (module seed, call counter).  The
    forward draws the mask in the Linear's epilogue, the backward regenerates it in the aggregation product's epilogue: if the
    two disagreed the loss and Z of step 1 would still match, the Adam update and everything after it would not."""
    from tests import dropout_mirror as DM
    from ultrafnd_git_amd.gcn import pretrain_gnn
    import torch.nn as nn
    z, n, sets, adj = _fixture()
    X = torch.from_numpy(z["X"])
    if n_nodes is not None:
        n, adj, X = n_nodes, np.ascontiguousarray(adj[:n_nodes, :n_nodes]), X[:n_nodes].contiguous()
    A = torch.from_numpy(adj)
    hid, p = 256, 0.2
    net = _gcn(z)
    head = nn.Linear(128, 1)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(z["head_w"])); head.bias.copy_(torch.from_numpy(z["head_b"]))
    assert net.dropout == p and net._calls == 0
    losses = pretrain_gnn(net, X.to(DEV), A.to(DEV), 128, epochs=2, head=head)
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    assert net.training
    Z = net(X.to(DEV), A.to(DEV)).cpu()
    assert net._calls == 3

    w0 = G.seeded_weights(int(z["weight_seed"]))

    def oracle(steps, ld=hid):
        m = [torch.from_numpy(DM.multipliers(net._seed, s, 9, p, n, hid, ld)) for s in steps]
        w2, ref_losses = G.pretrain(w0, X, A, torch.from_numpy(z["head_w"]), torch.from_numpy(z["head_b"]), epochs=2, drop_muls=m[:2])
        return w2, ref_losses, G.gcn_forward(w2, X, A, m[2])

    w2, ref_losses, ref_Z = oracle((1, 2, 3))
    err_loss = np.abs(np.asarray(losses) - np.asarray(ref_losses)).max()
    err_Z = (Z - ref_Z).abs().max().item()
    print(f"gcn train mode N={n}: loss err {err_loss:.2e}, train-mode Z err {err_Z:.2e}")
    assert err_loss <= 2e-6, (losses, ref_losses)
    for k in w2:
        upd_ref, upd = w2[k] - w0[k], sd[k] - w0[k]
        e = (upd - upd_ref).abs().max().item()
        print(f"  update {k}: err {e:.2e} (|update| max {upd_ref.abs().max().item():.2e})")
        assert e <= 2e-5 + 0.02 * upd_ref.abs().max().item(), k
    assert err_Z <= 1e-4
    # negative controls: the masks of the next call, and the element index built with another row stride
    for what, args in (("next step's masks", ((2, 3, 4),)), ("row stride hid + 4", ((1, 2, 3), hid + 4))):
        _, bad_losses, bad_Z = oracle(*args)
        frac = ((Z - bad_Z).abs() > 1e-4).float().mean().item()
        print(f"  control, {what}: Z differs beyond the bound on {frac:.3f} of the elements")
        assert frac >= 0.25, what
