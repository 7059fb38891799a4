#!/usr/bin/env python3
"""Mint tests/golden/recipe.npz from the REAL reference's FocalLoss, mixup_criterion and mixup_data
(src/training/run_train_eval.py:1245-1281).

Needs a checkout of the reference project (it is not part of this repository and never travels with it):

    python tests/golden/make_golden_recipe.py <path to the reference checkout>

The reference module imports torchvision at its top and nothing of it is used by the three functions: an empty stand-in module is
put into sys.modules before the import (the module's own fall-backs take care of whatever else is missing).  Data only:

  focal/logits (R, 2) fp32, focal/labels_a, focal/labels_b (R,) int64, focal/lam (fp32-exact), focal/alpha_gamma (6, 2) and, per
  (alpha, gamma) k:
    focal/k/rows          FocalLoss(alpha, gamma, reduction='none')(logits, labels_a)                                     (R,)
    focal/k/mean          FocalLoss(alpha, gamma)(logits, labels_a)                                                       ()
    focal/k/rows_mixed    mixup_criterion(FocalLoss(alpha, gamma, reduction='none'), logits, labels_a, labels_b, lam)    (R,)
    focal/k/mean_mixed    mixup_criterion(FocalLoss(alpha, gamma), logits, labels_a, labels_b, lam)                       ()
    focal/k/d, d_mixed    autograd d mean / d logits of the two means, on the rows with |gap| <= 12 only (focal/moderate: their
                          indices); the means these come from are taken over those rows alone
  The rows walk through the gaps 0, +-1e-3, +-1, +-12, +-30, +-100 three times, so that every gap meets both labels.
  mixup/x (B, W) fp32, mixup/y (B,), and what ONE seeded mixup_data(x, y, alpha=0.2) call returned: mixup/lam (float64), mixup/mixed,
  mixup/y_b -- and mixup/index, the permutation it drew, recovered by drawing torch.randperm(B) again from the same seed (asserted
  against y_b and the mixed rows).
"""
from __future__ import annotations

import os
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
GAPS = (0.0, 1e-3, -1e-3, 1.0, -1.0, 12.0, -12.0, 30.0, -30.0, 100.0, -100.0)
ALPHA_GAMMA = ((1.0, 2.0), (0.25, 2.0), (1.0, 1.0), (1.0, 3.5), (1.0, 5.0), (1.0, 0.0))
LAM = 0.3125          # exact in fp32, and so is 1 - lam
SEED = 20261021


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "src" / "training" / "run_train_eval.py").is_file():
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    sys.path.insert(0, str(ref))
    import torch
    import src.training.run_train_eval as T

    rng = np.random.default_rng(SEED)
    gap = np.array(GAPS * 3)
    R = gap.size
    logits = np.stack([np.zeros(R), -gap], 1).astype(np.float32)
    ya = np.concatenate([np.zeros(len(GAPS)), np.ones(len(GAPS)), rng.integers(0, 2, len(GAPS))]).astype(np.int64)
    yb = ya[rng.permutation(R)]
    moderate = np.flatnonzero(np.abs(gap) <= 12)
    store = {"focal/logits": logits, "focal/labels_a": ya, "focal/labels_b": yb, "focal/lam": np.float32(LAM), "focal/gap": gap,
             "focal/alpha_gamma": np.array(ALPHA_GAMMA), "focal/moderate": moderate}
    lg, ta, tb = torch.from_numpy(logits), torch.from_numpy(ya), torch.from_numpy(yb)
    for k, (alpha, gamma) in enumerate(ALPHA_GAMMA):
        rows, mean = T.FocalLoss(alpha, gamma, reduction="none"), T.FocalLoss(alpha, gamma)
        store[f"focal/{k}/rows"] = rows(lg, ta).numpy()
        store[f"focal/{k}/mean"] = mean(lg, ta).numpy()
        store[f"focal/{k}/rows_mixed"] = T.mixup_criterion(rows, lg, ta, tb, LAM).numpy()
        store[f"focal/{k}/mean_mixed"] = T.mixup_criterion(mean, lg, ta, tb, LAM).numpy()
        m = torch.from_numpy(moderate)
        for name, fn in (("d", lambda z: mean(z, ta[m])), ("d_mixed", lambda z: T.mixup_criterion(mean, z, ta[m], tb[m], LAM))):
            z = lg[m].clone().requires_grad_(True)
            fn(z).backward()
            store[f"focal/{k}/{name}"] = z.grad.numpy()
        print(f"alpha={alpha} gamma={gamma}: mean {float(store[f'focal/{k}/mean']):.6f} mixed {float(store[f'focal/{k}/mean_mixed']):.6f}")

    B, W = 9, 12
    x = (np.round(rng.normal(0, 1, (B, W)) * 1024) / 1024).astype(np.float32)
    y = rng.integers(0, 2, B).astype(np.int64)
    np.random.seed(SEED % 2 ** 31)
    torch.manual_seed(SEED)
    mixed, y_a, y_b, lam = T.mixup_data(torch.from_numpy(x), torch.from_numpy(y), alpha=0.2)
    torch.manual_seed(SEED)
    index = torch.randperm(B)
    assert torch.equal(y_a, torch.from_numpy(y)) and torch.equal(y_b, torch.from_numpy(y)[index])
    assert torch.equal(mixed, lam * torch.from_numpy(x) + (1 - lam) * torch.from_numpy(x)[index, :]) and 0.0 < lam < 1.0
    store.update({"mixup/x": x, "mixup/y": y, "mixup/lam": np.float64(lam), "mixup/index": index.numpy(), "mixup/mixed": mixed.numpy(),
                  "mixup/y_b": y_b.numpy()})
    print(f"mixup_data: lam {lam!r} index {index.tolist()}")
    path = HERE / "recipe.npz"
    np.savez_compressed(path, **store)
    assert path.stat().st_size < 100_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
