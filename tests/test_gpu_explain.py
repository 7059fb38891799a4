"""GPU: DeepTruthClassifier.feature_importance / explain_shap, explain.modality_attribution and ForensicTrainer.explain against the
float64 yardstick (tests/explain_ref.py) and the fixture minted from the reference's own classifier (tests/golden/explain.npz).

One criterion throughout, the project's gradient criterion (tests/test_gpu_sizes.py::test_tier_a_forward_backward_vs_oracle):
    max|a - r| / max(max|r|, ||r|| / sqrt(n), 1e-9) <= 5e-4.
Every test prints its worst value."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import explain_ref as X
from tests.helpers import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 5e-4
FEATS = ("text_features", "audio_features", "visual_features", "temporal_features", "gnn_feat")
# (hidden, trees, depth, aux); aux 0 = `use_aux: false`.  The shipped geometry, the same without aux, and tier_a_geom's first
GEOMS = {"default": (512, 6, 4, 2), "noaux": (512, 6, 4, 0), "H256-T16xD2-aux4": (256, 16, 2, 4)}


def _crit(a, r) -> float:
    a = torch.as_tensor(a).double().cpu()
    r = torch.as_tensor(r).double().cpu()
    assert a.shape == r.shape, (a.shape, r.shape)
    scale = max(r.abs().max().item(), r.norm().item() / max(1.0, r.numel() ** 0.5), 1e-9)
    e = (a - r).abs().max().item() / scale
    return float("inf") if e != e else e


def _clf(tmp_path, geom, seed=1234):
    """(module on the device in eval mode, its float32 parameter dict)"""
    from oracle import tier_a as O
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    H, T, D_, A = geom
    cy = tmp_path / f"classifier_{H}_{T}_{D_}_{A}.yaml"
    cy.write_text(f"input_dim: {H}\nhidden_dim: {H}\ndropout: 0.1\nnum_classes: 2\nuse_aux: {'true' if A else 'false'}\n"
                  f"aux_dim: {A or 2}\nnode_trees: {T}\nnode_depth: {D_}\nnode_tau: 10.0\ntemperature: 1.0\n")
    _, sd = O.seeded_params(seed, hidden=H, trees=T, depth=D_, aux_dim=A or 2, use_aux=A > 0)
    clf = DeepTruthClassifier(str(cy))
    assert clf.eff_aux == A and clf.hidden == H
    clf.load_state_dict(sd)
    return clf.to(DEV).eval(), sd


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


def _inputs(B, geom, seed):
    H, _, _, A = geom
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, generator=g) * 0.5, torch.rand(B, A or 2, generator=g)


# ------------------------------------------------------------------------------------------------ 1. feature_importance
@pytest.mark.parametrize("B", [1, 33, 256])
@pytest.mark.parametrize("name", list(GEOMS))
def test_feature_importance_vs_float64(tmp_path, name, B):
    geom = GEOMS[name]
    H, _, _, A = geom
    clf, sd = _clf(tmp_path, geom)
    fused, aux = _inputs(B, geom, 100 + B)
    worst = 0.0
    for c in (0, 1):
        imp, agg = clf.feature_importance(fused.to(DEV), aux.to(DEV), class_idx=c)
        assert imp.shape == (B, H + A) and agg.shape == (H + A,) and imp.device.type == "cuda" and agg.device.type == "cuda"
        r_imp, r_agg = X.feature_importance(_f64(sd), fused, aux, class_idx=c)
        worst = max(worst, _crit(imp, r_imp), _crit(agg, r_agg))
        imp2, none = clf.feature_importance(fused.to(DEV), aux.to(DEV), class_idx=c, aggregate=False)
        assert none is None and torch.equal(imp2, imp)
    print(f"feature_importance {name} B={B}: worst {worst:.3e} (<= {TOL:.0e})")
    assert worst <= TOL


def test_feature_importance_vs_the_reference_fixture(tmp_path):
    z = load_npz("explain.npz")
    clf, _ = _clf(tmp_path, GEOMS["noaux"], seed=int(z["param_seed"]))
    fused, aux = torch.from_numpy(z["fused"]).to(DEV), torch.from_numpy(z["aux"]).to(DEV)
    worst = 0.0
    for c in (0, 1):
        imp, agg = clf.feature_importance(fused, aux, class_idx=c)          # (aux is ignored with use_aux: false)
        imp_n, _ = clf.feature_importance(fused, None, class_idx=c)
        assert torch.equal(imp, imp_n)
        worst = max(worst, _crit(imp, z[f"fi_imp_c{c}"]), _crit(agg, z[f"fi_agg_c{c}"]))
    print(f"feature_importance vs the reference (use_aux: false, B=32): worst {worst:.3e} (<= {TOL:.0e})")
    assert worst <= TOL


def test_feature_importance_train_mode_without_dropout_equals_eval(tmp_path):
    clf, _ = _clf(tmp_path, GEOMS["default"])
    fused, aux = (t.to(DEV) for t in _inputs(33, GEOMS["default"], 7))
    imp_e, agg_e = clf.feature_importance(fused, aux)
    clf.train()
    imp_t1, _ = clf.feature_importance(fused, aux)
    imp_t2, _ = clf.feature_importance(fused, aux)
    assert not torch.equal(imp_t1, imp_t2) and not torch.equal(imp_t1, imp_e)      # dropout is live: two calls differ, as in the reference
    clf.dropout = clf.node_dropout = 0.0
    imp_t, agg_t = clf.feature_importance(fused, aux)
    assert clf.training and torch.equal(imp_t, imp_e) and torch.equal(agg_t, agg_e)


# ------------------------------------------------------------------------------------------------ 2. explain_shap
def test_explain_shap_vs_the_reference_fixture(tmp_path):
    z = load_npz("explain.npz")
    clf, _ = _clf(tmp_path, GEOMS["default"], seed=int(z["param_seed"]))
    clf.train()
    noise = torch.randn(X.STEPS, 32, 514, generator=torch.Generator().manual_seed(int(z["noise_seed"])))
    assert abs(float(noise.double().sum()) - float(z["noise_checksum"])) <= 1e-9
    res = clf.explain_shap(torch.from_numpy(z["fused"]).to(DEV), torch.from_numpy(z["aux"]).to(DEV), noise=noise.to(DEV))
    assert res["method"] == "smooth-grad" and isinstance(res["values"], np.ndarray) and res["values"].dtype == np.float32
    assert res["values"].shape == (32, 514) and not clf.training
    e = _crit(res["values"], z["sg_values"])
    print(f"explain_shap vs the reference (B=32, its noise): {e:.3e} (<= {TOL:.0e})")
    assert e <= TOL


@pytest.mark.parametrize("name,B", [("default", 2), ("default", 300), ("noaux", 33), ("H256-T16xD2-aux4", 33)])
def test_explain_shap_vs_float64(tmp_path, name, B):
    geom = GEOMS[name]
    H, _, _, A = geom
    clf, sd = _clf(tmp_path, geom)
    fused, aux = _inputs(B, geom, 200 + B)
    n = min(B, 256)
    noise = torch.randn(X.STEPS, n, H + A, generator=torch.Generator().manual_seed(300 + B))
    res = clf.explain_shap(fused.to(DEV), aux.to(DEV), noise=noise.to(DEV))
    assert res["values"].shape == (n, H + A)
    ref = X.smooth_grad(_f64(sd), fused, aux, noise)
    e = _crit(res["values"], ref)
    miss = _crit(res["values"], X.smooth_grad(_f64(sd), fused, aux, noise, walk=False))
    print(f"explain_shap {name} B={B}: {e:.3e} (<= {TOL:.0e}); against independent perturbations {miss:.3e}")
    assert e <= TOL
    assert miss > 20 * TOL          # the comparison can see the walk


def test_explain_shap_in_chunks_of_whole_steps(tmp_path):
    """16 x 4,200 = 67,200 rows exceed one call's 65,536: 15 steps, then 1."""
    geom = GEOMS["default"]
    clf, sd = _clf(tmp_path, geom)
    n = 4200
    fused, aux = _inputs(n, geom, 5)
    noise = torch.randn(X.STEPS, n, 514, generator=torch.Generator().manual_seed(6))
    res = clf.explain_shap(fused.to(DEV), aux.to(DEV), max_samples=n, noise=noise.to(DEV))
    assert res["values"].shape == (n, 514) and np.isfinite(res["values"]).all()
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(8))[:64].tolist()
    ref = X.smooth_grad(_f64(sd), fused, aux, noise, max_samples=n, rows=rows)
    e = _crit(res["values"][rows], ref)
    print(f"explain_shap B'=4200 in two chunks, 64 sampled rows: {e:.3e} (<= {TOL:.0e})")
    assert e <= TOL
    assert clf._xws is None or clf._xws[1].numel() <= clf.XWS_KEEP_FLOATS      # the gigabyte workspace of the first chunk is not kept


def test_explain_shap_default_noise(tmp_path):
    clf, _ = _clf(tmp_path, GEOMS["default"])
    clf.train()
    fused, aux = (t.to(DEV) for t in _inputs(40, GEOMS["default"], 9))
    res = clf.explain_shap(fused, aux, max_samples=24)
    v = res["values"]
    assert res["method"] == "smooth-grad" and v.shape == (24, 514) and v.dtype == np.float32
    assert np.isfinite(v).all() and (v >= 0).all() and v.max() > 0 and not clf.training


# ------------------------------------------------------------------------------------------------ 3. modality_attribution
def _head(use_gnn=True, seed=1234):
    from oracle import tier_a as O
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.fusion import CrossModalTransformer
    fus_sd, clf_sd = O.seeded_params(seed, use_gnn=use_gnn)
    fusion = CrossModalTransformer("configs/model_configs/fusion.yaml" if use_gnn else "configs/model_configs/fusion_nognn.yaml")
    clf = DeepTruthClassifier()
    fusion.load_state_dict(fus_sd); clf.load_state_dict(clf_sd)
    return fusion.to(DEV).eval(), clf.to(DEV).eval(), fus_sd, clf_sd


@pytest.mark.parametrize("B,use_gnn", [(1, True), (33, True), (256, True), (33, False)])
def test_modality_attribution_vs_float64(B, use_gnn):
    from oracle import tier_a as O
    from ultrafnd_git_amd import _lib as L
    from ultrafnd_git_amd.explain import modality_attribution
    fusion, clf, fus_sd, clf_sd = _head(use_gnn)
    batch = O.seeded_batch(50 + B, B)
    gb = {k: v.to(DEV) for k, v in batch.items()}
    worst = 0.0
    for c in (1, 0):
        out = modality_attribution(fusion, clf, {k: gb[k] for k in FEATS}, gb["aux"], class_idx=c)
        ref = X.modality_attribution(_f64(fus_sd), _f64(clf_sd), batch, class_idx=c)
        names = [n for n in X.INPUTS if use_gnn or n != "gnn_feat"]
        assert list(out["order"]) == names == list(ref) and sorted(out["inputs"]) == sorted(names)
        assert out["modality"].shape == (B, len(names))
        for i, n in enumerate(names):
            e = _crit(out["inputs"][n], ref[n])
            worst = max(worst, e)
            assert e <= TOL, (n, e)
            assert torch.equal(out["modality"][:, i], out["inputs"][n].sum(dim=1)), n
    print(f"modality_attribution B={B} use_gnn={use_gnn}: worst {worst:.3e} (<= {TOL:.0e})")
    # the older two entries return the bits of ufnd_fusion_input_grads for their outputs (the workspace still holds this backward)
    lib, d, s = L.lib(), fusion.dims(), L.stream_ptr(torch.device(DEV))
    ws, st, pt = fusion.workspace(B, True).data_ptr(), fusion.rng().ptr, fusion.param_table()
    widths = (768, 128, 512, 256, 128)
    new = [torch.full((B, w), float("nan"), device=DEV) for w in widths]
    L.check(lib.ufnd_fusion_input_grads(C.byref(d), C.byref(pt), ws, B, *[t.data_ptr() for t in new[:4]], new[4].data_ptr() if use_gnn else None,
                                        st, s), "ufnd_fusion_input_grads")
    old = [torch.full((B, w), float("nan"), device=DEV) for w in widths]
    L.check(lib.ufnd_fusion_feature_grads(C.byref(d), C.byref(pt), ws, B, old[0].data_ptr(), old[2].data_ptr(), st, s), "ufnd_fusion_feature_grads")
    assert torch.equal(old[0], new[0]) and torch.equal(old[2], new[2]) and not torch.isnan(new[1]).any() and not torch.isnan(new[3]).any()
    if use_gnn:
        L.check(lib.ufnd_fusion_gnn_input_grad(C.byref(d), C.byref(pt), ws, B, old[4].data_ptr(), st, s), "ufnd_fusion_gnn_input_grad")
        assert torch.equal(old[4], new[4])
    else:
        assert lib.ufnd_fusion_input_grads(C.byref(d), C.byref(pt), ws, B, None, None, None, None, new[4].data_ptr(), st, s) == 1
    one_text = torch.empty(B, 768, device=DEV)
    L.check(lib.ufnd_fusion_feature_grads(C.byref(d), C.byref(pt), ws, B, one_text.data_ptr(), None, st, s), "ufnd_fusion_feature_grads")
    assert torch.equal(one_text, new[0])


def test_modality_attribution_keeps_the_stale_activation_guard_honest():
    from oracle import tier_a as O
    from ultrafnd_git_amd.explain import modality_attribution
    fusion, clf, _, _ = _head()
    gb = {k: v.to(DEV) for k, v in O.seeded_batch(3, 4).items()}
    fo = fusion({k: gb[k] for k in FEATS})
    modality_attribution(fusion, clf, {k: gb[k] for k in FEATS}, gb["aux"])      # overwrites the B = 4 grad workspace
    with pytest.raises(RuntimeError, match="overwritten"):
        fo["fused"].sum().backward()


# ------------------------------------------------------------------------------------------------ 4. nothing leaks
def test_identical_calls_return_identical_bits(tmp_path):
    from oracle import tier_a as O
    from ultrafnd_git_amd.explain import modality_attribution
    fusion, clf, _, _ = _head()
    gb = {k: v.to(DEV) for k, v in O.seeded_batch(21, 33).items()}
    fused = fusion({k: gb[k] for k in FEATS})["fused"].detach()
    noise = torch.randn(X.STEPS, 33, 514, generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b = clf.feature_importance(fused, gb["aux"]), clf.feature_importance(fused, gb["aux"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = clf.explain_shap(fused, gb["aux"], noise=noise), clf.explain_shap(fused, gb["aux"], noise=noise)
    assert np.array_equal(a["values"], b["values"])
    a = modality_attribution(fusion, clf, {k: gb[k] for k in FEATS}, gb["aux"])
    b = modality_attribution(fusion, clf, {k: gb[k] for k in FEATS}, gb["aux"])
    assert all(torch.equal(a["inputs"][n], b["inputs"][n]) for n in a["order"]) and torch.equal(a["modality"], b["modality"])


@pytest.mark.parametrize("train", [False, True])
def test_explanations_leave_parameters_gradients_and_pending_backwards_alone(tmp_path, train):
    clf, _ = _clf(tmp_path, GEOMS["default"])
    B = 33
    fused, aux = (t.to(DEV) for t in _inputs(B, GEOMS["default"], 11))
    y = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(2)).to(DEV)

    def run(explain: bool):
        torch.manual_seed(77)
        clf._on_rehome()                    # fresh workspaces and step states: both runs start from the same dropout key
        clf.train(train)
        x = fused.clone().requires_grad_(True)
        out = clf(x, aux)
        if explain:
            params, grads = clf._arena.data.clone(), clf._arena.ensure_grad().clone()
            clf.feature_importance(fused, aux)                      # the same batch size as the pending backward
            clf.feature_importance(fused, aux, class_idx=0, aggregate=False)
            assert torch.equal(params, clf._arena.data) and torch.equal(grads, clf._arena.ensure_grad())
            if not train:       # (explain_shap leaves the module in eval mode by design: between a train-mode forward and its
                clf.explain_shap(fused, aux)      # backward it would not change the gradients either, but the mode)
                assert torch.equal(params, clf._arena.data) and torch.equal(grads, clf._arena.ensure_grad())
        F.cross_entropy(out["logits"], y).backward()
        res = x.grad.clone(), clf._arena.ensure_grad().clone(), out["logits"].detach().clone()
        if explain:             # after the backward, in either mode: explain_shap writes neither parameters nor gradients
            params = clf._arena.data.clone()
            clf.explain_shap(fused, aux)
            assert torch.equal(params, clf._arena.data) and torch.equal(res[1], clf._arena.ensure_grad())
        return res

    clf._arena.ensure_grad().fill_(0.25)
    plain, explained = run(False), run(True)
    assert all(torch.equal(p, e) for p, e in zip(plain, explained))
    assert plain[1].abs().sum() > 0


def _trainer(tmp_path, B, use_graph, n=64, **kw):
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=B, device=DEV, use_graph=use_graph, **kw)
    return ForensicTrainer(cfg, cache=synthetic_cache(n, seed=3))


def test_explanations_between_train_steps_change_nothing(tmp_path):
    res = []
    for explain in (False, True):
        torch.manual_seed(5)
        tr = _trainer(tmp_path, 16, True)
        tr.fusion.train(); tr.clf.train()
        it = iter(tr.train_loader)
        for step in range(3):
            out = tr.train_step(next(it))
            if explain and step < 2:
                e = tr.explain(split="train", max_samples=16)        # the train step's own batch size: its buffers are not these
                assert tr.fusion.training and tr.clf.training and e["modality"].shape[0] == 16
                g = torch.Generator().manual_seed(step)
                tr.clf.explain_shap(torch.randn(16, 512, generator=g).to(DEV), torch.rand(16, 2, generator=g).to(DEV))
                assert not tr.clf.training
                tr.clf.train()
        res.append((out["logits"].clone(), float(out["loss"].cpu()), tr.arena.data.clone()))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and torch.equal(res[0][2], res[1][2])


# ------------------------------------------------------------------------------------------------ 5. ForensicTrainer.explain
def test_trainer_explain(tmp_path):
    from ultrafnd_git_amd.explain import modality_attribution
    tr = _trainer(tmp_path, 16, True)
    tr.fusion.train(); tr.clf.eval()
    ds = tr._dataset("test")
    n = min(len(ds), 5)
    out = tr.explain(split="test", max_samples=5, class_idx=0)
    assert tr.fusion.training and not tr.clf.training                  # the modes it found
    assert out["order"] == X.INPUTS and out["modality"].shape == (n, 6)
    assert torch.equal(out["index"], torch.arange(n, device=out["index"].device))
    widths = dict(zip(X.INPUTS, (768, 128, 512, 256, 128, 2)))
    assert all(out["inputs"][k].shape == (n, w) for k, w in widths.items())
    feats = {"text_features": ds.T[:n], "audio_features": ds.A[:n], "visual_features": ds.V[:n], "temporal_features": ds.U[:n],
             "gnn_feat": ds.G[:n]}
    direct = modality_attribution(tr.fusion, tr.clf, feats, ds.AUX[:n], class_idx=0)
    assert all(torch.equal(out["inputs"][k], direct["inputs"][k]) for k in X.INPUTS) and torch.equal(out["modality"], direct["modality"])
    whole = tr.explain(split="val")
    assert whole["modality"].shape[0] == min(len(tr._dataset("val")), 256)
    tr.cfg.gnn_in_graph = True
    with pytest.raises(NotImplementedError, match="gnn_in_graph"):
        tr.explain()
    tr.cfg.gnn_in_graph = False
    tr.cfg.encode_inline = True
    with pytest.raises(NotImplementedError, match="encoder-fed"):
        tr.explain()
