"""CPU: the explanation yardstick (tests/explain_ref.py) against the fixture minted from the reference's own classifier
(tests/golden/explain.npz, tests/golden/make_golden_explain.py), the four C entries, and the argument checks of
DeepTruthClassifier.feature_importance / explain_shap -- which run before anything needs a device."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import explain_ref as X
from tests.helpers import load_npz

REPO = Path(__file__).resolve().parents[1]
ENTRIES = ("ufnd_classifier_input_grad", "ufnd_smoothgrad_points", "ufnd_attribution_reduce", "ufnd_fusion_input_grads")


def _fixture():
    from oracle import tier_a as O
    z = load_npz("explain.npz")
    _, clf = O.seeded_params(int(z["param_seed"]))
    _, clf0 = O.seeded_params(int(z["param_seed"]), use_aux=False)
    assert abs(float(sum(v.double().sum() for v in clf.values())) - float(z["param_checksum"])) <= 1e-9
    assert abs(float(sum(v.double().sum() for v in clf0.values())) - float(z["param_checksum_noaux"])) <= 1e-9
    fused, aux = torch.from_numpy(z["fused"]), torch.from_numpy(z["aux"])
    noise = torch.randn(X.STEPS, fused.shape[0], 514, generator=torch.Generator().manual_seed(int(z["noise_seed"])))
    assert abs(float(noise.double().sum()) - float(z["noise_checksum"])) <= 1e-9
    return z, clf, clf0, fused, aux, noise


def _rel_l2(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float(np.linalg.norm(a - r) / np.linalg.norm(r))


def test_smooth_grad_yardstick_reproduces_the_reference():
    z, clf, _, fused, aux, noise = _fixture()
    ref = z["sg_values"]
    assert ref.shape == (32, 514) and ref.dtype == np.float32
    e32 = float(np.abs(X.smooth_grad(clf, fused, aux, noise).numpy() - ref).max())
    r64 = _rel_l2(X.smooth_grad({k: v.double() for k, v in clf.items()}, fused, aux, noise).numpy(), ref)
    print(f"smooth-grad: float32 max-abs {e32:.3e} (<= 1e-6), float64 rel-L2 {r64:.3e} (<= 1e-6)")
    assert e32 <= 1e-6 and r64 <= 1e-6


def test_the_yardstick_can_tell_the_walk_from_independent_perturbations():
    z, clf, _, fused, aux, noise = _fixture()
    r = _rel_l2(X.smooth_grad(clf, fused, aux, noise, walk=False).numpy(), z["sg_values"])
    print(f"independent perturbations vs the reference's walk: rel-L2 {r:.3e} (> 1e-2)")
    assert r > 1e-2


def test_smooth_grad_rows_subset_equals_the_full_run():
    """(float64, to rounding: a BLAS product's summation order may depend on the number of rows)"""
    _, clf, _, fused, aux, noise = _fixture()
    clf = {k: v.double() for k, v in clf.items()}
    rows = [0, 5, 31]
    full = X.smooth_grad(clf, fused, aux, noise)
    assert torch.allclose(X.smooth_grad(clf, fused, aux, noise, rows=rows), full[rows], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("c", [0, 1])
def test_feature_importance_yardstick_reproduces_the_reference(c):
    z, _, clf0, fused, aux, _ = _fixture()
    imp, agg = X.feature_importance(clf0, fused, aux, class_idx=c)           # (aux is ignored without aux columns in pre.0)
    e32 = max(float(np.abs(imp.numpy() - z[f"fi_imp_c{c}"]).max()), float(np.abs(agg.numpy() - z[f"fi_agg_c{c}"]).max()))
    i64, a64 = X.feature_importance({k: v.double() for k, v in clf0.items()}, fused, None, class_idx=c)
    r64 = max(_rel_l2(i64.numpy(), z[f"fi_imp_c{c}"]), _rel_l2(a64.numpy(), z[f"fi_agg_c{c}"]))
    print(f"feature_importance class {c}: float32 max-abs {e32:.3e} (<= 1e-6), float64 rel-L2 {r64:.3e} (<= 1e-6)")
    assert imp.shape == (32, 512) and agg.shape == (512,) and e32 <= 1e-6 and r64 <= 1e-6


def test_modality_attribution_yardstick_is_gradient_times_input_through_both_modules():
    """Its sum over a row's inputs is what a first-order expansion would assign; checked here only for shape, sign and the
    aux part, which must equal the classifier-only yardstick's aux columns."""
    from oracle import tier_a as O
    fus, clf = O.seeded_params(1234)
    batch = O.seeded_batch(5, 3)
    out = X.modality_attribution(fus, clf, batch, class_idx=1)
    assert list(out) == list(X.INPUTS) and all((v >= 0).all() and v.shape == batch[k].shape for k, v in out.items())
    with torch.no_grad():
        fused = O.forward_batch(fus, clf, batch)["fused"]
    imp, _ = X.feature_importance(clf, fused, batch["aux"], class_idx=1)
    assert float((imp[:, 512:] - out["aux"]).abs().max()) <= 1e-6
    fus0, _ = O.seeded_params(1234, use_gnn=False)
    assert "gnn_feat" not in X.modality_attribution(fus0, clf, batch)


def test_header_declares_and_library_exports_the_four_entries():
    import torch  # noqa: F401  (its HIP runtime must be resident before ours is resolved)
    from ultrafnd_git_amd.build import build
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "ultrafnd_hip.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(build()))
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert hasattr(lib, name), name
    from ultrafnd_git_amd import _lib as L
    for name in ENTRIES:
        assert getattr(L.lib(), name).argtypes, name
    assert L.lib().ufnd_abi_version() == 6


def test_entry_argument_checks_without_a_gpu():
    from ultrafnd_git_amd import _lib as L
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    lib, d = L.lib(), DeepTruthClassifier().dims()
    one = ctypes.c_void_p(256)
    assert lib.ufnd_classifier_input_grad(ctypes.byref(d), None, None, 512, None, 4, 0, 0, 1, None, None, 516, None, None, None, None) == 1
    assert b"null" in lib.ufnd_last_error()
    assert lib.ufnd_smoothgrad_points(ctypes.byref(d), one, 516, one, one, 516, 4200, 16, 0, 16, one, None) == 1
    assert b"65536" in lib.ufnd_last_error()
    assert lib.ufnd_smoothgrad_points(ctypes.byref(d), one, 514, one, one, 516, 4, 16, 0, 16, one, None) == 1
    assert lib.ufnd_attribution_reduce(2, one, 516, None, 0, 4, 514, 1, 0, 0, one, 516, None, None, None) == 1
    assert lib.ufnd_attribution_reduce(1, one, 516, None, 0, 4, 514, 1, 0, 0, one, 516, None, None, None) == 1      # grad x input without X
    assert lib.ufnd_attribution_reduce(0, one, 512, None, 0, 4, 514, 1, 0, 0, one, 516, None, None, None) == 1     # ldg < W
    assert lib.ufnd_fusion_input_grads(ctypes.byref(d), None, None, 4, None, None, None, None, None, None, None) == 1


def test_a_cpu_resident_classifier_refuses_to_explain():
    from ultrafnd_git_amd._lib import UltrafndHipError
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    clf = DeepTruthClassifier().train()
    fused, aux = torch.randn(4, 512), torch.rand(4, 2)
    with pytest.raises(UltrafndHipError, match="no CPU fallback"):
        clf.feature_importance(fused, aux)
    with pytest.raises(UltrafndHipError, match="no CPU fallback"):
        clf.explain_shap(fused, aux)
    assert clf.training            # a refused call changes nothing, the mode included


def test_argument_checks_by_name(tmp_path):
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    clf = DeepTruthClassifier()
    fused, aux = torch.randn(4, 512), torch.rand(4, 2)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="class_idx"):
            clf.feature_importance(fused, aux, class_idx=bad)
    with pytest.raises(RuntimeError, match="fused"):
        clf.feature_importance(torch.randn(4, 500), aux)
    with pytest.raises(RuntimeError, match="fused"):
        clf.explain_shap(torch.randn(4, 514), aux)
    with pytest.raises(RuntimeError, match="aux"):
        clf.feature_importance(fused, torch.rand(4, 3))
    with pytest.raises(RuntimeError, match="aux is required"):
        clf.feature_importance(fused)
    with pytest.raises(RuntimeError, match="aux is required"):
        clf.explain_shap(fused)
    with pytest.raises(ValueError, match="B >= 2"):
        clf.explain_shap(fused[:1], aux[:1])
    with pytest.raises(ValueError, match="B >= 2"):
        clf.explain_shap(fused, aux, max_samples=1)
    for shape in ((16, 4, 512), (15, 4, 514), (16, 3, 514), (16, 4 * 514)):
        with pytest.raises(ValueError, match="noise"):
            clf.explain_shap(fused, aux, noise=torch.zeros(*shape))
    with pytest.raises(ValueError, match="noise"):
        clf.explain_shap(torch.randn(300, 512), torch.rand(300, 2), noise=torch.zeros(16, 300, 514))      # 256 rows are explained
    cy = tmp_path / "classifier.yaml"
    cy.write_text("input_dim: 512\nhidden_dim: 512\ndropout: 0.1\nnum_classes: 2\nuse_aux: false\naux_dim: 2\n"
                  "node_trees: 6\nnode_depth: 4\nnode_tau: 10.0\ntemperature: 1.0\n")
    clf0 = DeepTruthClassifier(str(cy))
    with pytest.raises(ValueError, match="noise"):
        clf0.explain_shap(fused, aux, noise=torch.zeros(16, 4, 514))      # use_aux: false explains the 512 fused columns


def test_modality_attribution_and_trainer_checks_without_a_gpu():
    from ultrafnd_git_amd._lib import UltrafndHipError
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.explain import modality_attribution
    from ultrafnd_git_amd.fusion import CrossModalTransformer
    from ultrafnd_git_amd.trainer import ForensicTrainer
    from oracle import tier_a as O
    fusion, clf = CrossModalTransformer(), DeepTruthClassifier()
    batch = O.seeded_batch(5, 3)
    with pytest.raises(ValueError, match="class_idx"):
        modality_attribution(fusion, clf, batch, batch["aux"], class_idx=3)
    with pytest.raises(RuntimeError, match="gnn_feat"):
        modality_attribution(fusion, clf, {k: v for k, v in batch.items() if k != "gnn_feat"}, batch["aux"])
    with pytest.raises(UltrafndHipError, match="no CPU fallback"):
        modality_attribution(fusion, clf, batch, batch["aux"])
    assert callable(ForensicTrainer.explain)
