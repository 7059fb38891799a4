"""Mints tests/golden/explain.npz from the REAL reference classifier (src/models/fusion/deep_truth_classifier.py:189-272), the way
make_golden.py mints the other fixtures: `transformers` masked, parameters from oracle.tier_a.seeded_params(1234), a temporary
YAML for `use_aux: false`.  Run from the repository root with the reference checkout at REF:

    python tests/golden/make_golden_explain.py

  (a) explain_shap -- its smooth-grad branch (`shap` is not installed) -- for B = 32 with the shipped classifier.yaml; the
      reference's torch.randn_like is replaced for the call by the draws of torch.randn(16, 32, 514, generator=manual_seed(s));
  (b) feature_importance, classes 0 and 1, on the `use_aux: false` build (with the shipped `use_aux: true` the reference's method
      cannot return: it reads .grad of the non-leaf cat result, or feeds 512 columns to the 514-wide pre.0).

Stored: fused, aux, the outputs, the seeds, and checksums of parameters and noise (not the noise, not the weights).  Before it
writes, the script asserts that tests/explain_ref.py (float32) equals the reference within 1e-6.  No test reads the reference.
"""
from __future__ import annotations

import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
REF = Path("/root/reference")
sys.path.insert(0, str(REPO))

PARAM_SEED, BATCH_SEED, NOISE_SEED, B = 1234, 13, 77, 32


def main():
    sys.modules["transformers"] = None
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    os.chdir(REF)
    from src.models.fusion.deep_truth_classifier import DeepTruthClassifier
    from oracle import tier_a as O
    from tests import explain_ref as X

    fus_sd, clf_sd = O.seeded_params(PARAM_SEED)
    batch = O.seeded_batch(BATCH_SEED, B)
    with torch.no_grad():
        fused = O.forward_batch(fus_sd, clf_sd, batch, train=False)["fused"].contiguous()      # realistic classifier inputs
    aux = batch["aux"]
    store = {"param_seed": np.int64(PARAM_SEED), "batch_seed": np.int64(BATCH_SEED), "noise_seed": np.int64(NOISE_SEED),
             "fused": fused.numpy(), "aux": aux.numpy(),
             "param_checksum": np.float64(sum(v.double().sum() for v in clf_sd.values()))}

    # ---- (a) smooth-grad, shipped YAML
    torch.manual_seed(0)
    clf = DeepTruthClassifier("configs/model_configs/classifier.yaml").to("cpu")
    assert list(clf.state_dict().keys()) == list(clf_sd.keys())
    clf.load_state_dict(clf_sd)
    clf.train()
    noise = torch.randn(X.STEPS, B, 514, generator=torch.Generator().manual_seed(NOISE_SEED))
    draws = iter(noise)
    real = torch.randn_like
    torch.randn_like = lambda t, *a, **k: next(draws).to(t.dtype)
    try:
        res = clf.explain_shap(fused, aux, max_samples=256)
    finally:
        torch.randn_like = real
    assert res["method"] == "smooth-grad" and not clf.training and next(draws, None) is None      # all 16 draws taken, eval mode kept
    vals = np.asarray(res["values"], dtype=np.float32)
    assert vals.shape == (B, 514) and np.isfinite(vals).all()
    mine = X.smooth_grad(clf_sd, fused, aux, noise).numpy()
    err = float(np.abs(mine - vals).max())
    assert err <= 1e-6, err
    f64 = X.smooth_grad({k: v.double() for k, v in clf_sd.items()}, fused, aux, noise).numpy()
    rel64 = float(np.linalg.norm(f64 - vals) / np.linalg.norm(vals))
    indep = X.smooth_grad(clf_sd, fused, aux, noise, walk=False).numpy()
    rel_indep = float(np.linalg.norm(indep - vals) / np.linalg.norm(vals))
    print(f"smooth-grad: restatement vs reference max-abs {err:.3e}; float64 rel-L2 {rel64:.3e}; independent perturbations rel-L2 {rel_indep:.3e}")
    assert rel64 <= 1e-6 and rel_indep > 1e-2
    store["sg_values"] = vals
    store["noise_checksum"] = np.float64(noise.double().sum())

    # ---- (b) feature_importance on the use_aux: false build
    tmp = Path(tempfile.mkdtemp())
    cy = tmp / "classifier_noaux.yaml"
    cy.write_text("input_dim: 512\nhidden_dim: 512\ndropout: 0.1\nnum_classes: 2\nuse_aux: false\naux_dim: 2\n"
                  "node_trees: 6\nnode_depth: 4\nnode_tau: 10.0\ntemperature: 1.0\n")
    _, clf0_sd = O.seeded_params(PARAM_SEED, use_aux=False)
    torch.manual_seed(0)
    clf0 = DeepTruthClassifier(str(cy)).to("cpu")
    assert list(clf0.state_dict().keys()) == list(clf0_sd.keys()) and clf0.state_dict()["pre.0.weight"].shape == (512, 512)
    clf0.load_state_dict(clf0_sd)
    clf0.eval()
    store["param_checksum_noaux"] = np.float64(sum(v.double().sum() for v in clf0_sd.values()))
    for c in (0, 1):
        # (fresh copies: the reference turns the tensor it is given into a leaf whose .grad accumulates over calls)
        imp, agg = clf0.feature_importance(fused.clone(), None, class_idx=c, aggregate=True)
        imp2, none = clf0.feature_importance(fused.clone(), aux.clone(), class_idx=c, aggregate=False)      # a given aux is ignored
        assert none is None and torch.equal(imp, imp2)
        mi, ma = X.feature_importance(clf0_sd, fused, None, class_idx=c)
        e = max(float((mi - imp.detach()).abs().max()), float((ma - agg.detach()).abs().max()))
        print(f"feature_importance class {c}: restatement vs reference max-abs {e:.3e}")
        assert e <= 1e-6, e
        store[f"fi_imp_c{c}"] = imp.detach().numpy()
        store[f"fi_agg_c{c}"] = agg.detach().numpy()
    out = HERE / "explain.npz"
    np.savez_compressed(out, **store)
    print(out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
