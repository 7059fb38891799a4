"""Shared test helpers: fixture loading and digest comparison (tests only)."""
import json
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"


def load_npz(name):
    return np.load(GOLDEN / name, allow_pickle=False)


def digest(t: torch.Tensor):
    f = t.detach().double().flatten().cpu()
    n = f.numel()
    stride = max(1, n // 16)
    return {"norm": f.norm().item(), "sum": f.sum().item(),
            "head": f[:16].float().numpy(), "strided": f[::stride][:16].float().numpy()}


def assert_digest_close(z, prefix, t, rtol, atol, what=""):
    """Compare tensor t with the digest stored under `prefix` in npz z."""
    d = digest(t)
    ref_norm = float(z[f"{prefix}/norm"])
    scale = max(ref_norm / max(1.0, np.sqrt(t.numel())), 1e-12)   # rms of the reference tensor
    assert abs(d["norm"] - ref_norm) <= rtol * ref_norm + atol, (what, prefix, "norm", d["norm"], ref_norm)
    for k in ("head", "strided"):
        ref = z[f"{prefix}/{k}"]
        err = np.abs(d[k] - ref).max()
        assert err <= rtol * max(np.abs(ref).max(), scale) + atol, (what, prefix, k, err)


def nograd_keys(z):
    return json.loads(str(z["nograd_keys"]))


def feature_errors(got, ref):
    """Three views of the error of unit-norm feature rows (max-abs alone lets a 3x regression pass):
    max-abs, the worst row's relative L2 error ||got - ref|| / ||ref||, and the worst row's 1 - cosine."""
    g = torch.as_tensor(np.asarray(got) if not torch.is_tensor(got) else got).double().cpu()
    r = torch.as_tensor(np.asarray(ref) if not torch.is_tensor(ref) else ref).double().cpu()
    g, r = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
    d = g - r
    cos = (g * r).sum(-1) / (g.norm(dim=-1) * r.norm(dim=-1)).clamp_min(1e-30)
    return {"max_abs": d.abs().max().item(), "rel_l2": (d.norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-30)).max().item(),
            "one_minus_cos": (1.0 - cos).max().item()}


def assert_features_close(got, ref, max_abs, rel_l2, one_minus_cos, what=""):
    e = feature_errors(got, ref)
    print(f"{what}: max-abs {e['max_abs']:.3e} (<= {max_abs:.1e}), rel-L2 {e['rel_l2']:.3e} (<= {rel_l2:.1e}), "
          f"1-cos {e['one_minus_cos']:.3e} (<= {one_minus_cos:.1e})")
    assert e["max_abs"] <= max_abs and e["rel_l2"] <= rel_l2 and e["one_minus_cos"] <= one_minus_cos, (what, e)
    return e


def hidden_errors(got, ref):
    """Hidden states (entries of order 1): relative RMS error and max-abs."""
    g, r = got.double().cpu(), ref.double().cpu()
    d = g - r
    return {"rel_rms": (d.pow(2).mean().sqrt() / r.pow(2).mean().sqrt()).item(), "max_abs": d.abs().max().item()}


def outlier_text_problem(gain: float):
    """The outlier-shaped 4-layer BERT of tests/test_gpu_encoder_train.py (four hidden dimensions with `gain` x LayerNorm gains, every
    LayerNorm bias offset by half a standard deviation) and its token batch: (weights, ids, mask, loss seed)."""
    from oracle import encoders_ref as E
    w = E.seeded_weights(E.bert_shapes(layers=4, vocab=800), 93)
    hot = [7, 300, 511, 640]
    for k in list(w):
        if k.endswith("LayerNorm.weight"):
            w[k] = w[k].clone()
            w[k][hot] *= gain
        if k.endswith("LayerNorm.bias"):
            w[k] = w[k] + 0.5
    ids, mask = E.synthetic_tokens(193, 4, 96, vocab=800)
    return w, ids, mask, 7


def grad_rel_errors(got: dict, ref: dict, floor_frac: float = 2e-3):
    """Relative L2 error of every gradient tensor of `got` against `ref`, and the absolute floor test_gpu_encoder_train.py's
    _compare grants a tensor whose own gradient is (nearly) zero: floor_frac x the largest per-element gradient scale x sqrt(numel).
    Returns ({name: (rel, err, floor, ref norm)}, worst rel over the tensors whose error exceeds their floor, its name)."""
    top = max(g.norm().item() / max(1, g.numel()) ** 0.5 for g in ref.values())
    out, worst = {}, ("", 0.0)
    for k, r in ref.items():
        err = (got[k].double() - r.double()).norm().item()
        rn = r.double().norm().item()
        rel = err / max(rn, 1e-30)
        floor = floor_frac * top * max(1, r.numel()) ** 0.5
        out[k] = (rel, err, floor, rn)
        if err > floor and rel > worst[1]:
            worst = (k, rel)
    return out, worst[1], worst[0]


def qk_weight_rel_l2(got: dict, ref: dict) -> float:
    """Relative L2 error of all query / key weight gradients taken together (the tensors a saturated softmax hits)."""
    num = den = 0.0
    for k, r in ref.items():
        if k.endswith(("attention.self.query.weight", "attention.self.key.weight")):
            num += float((got[k].double() - r.double()).pow(2).sum())
            den += float(r.double().pow(2).sum())
    return (num / max(den, 1e-300)) ** 0.5
