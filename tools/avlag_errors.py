#!/usr/bin/env python3
"""Measured figures of the A/V lag kernels (ultrafnd_git_amd/temporal.py: av_lag, csrc/av_lag.hip) against tests/avlag_ref.py.

    avlag_errors.py [--out profiles/avlag_errors.txt]
        per case of tests/golden/avlag.npz and per seeded pair at n = 2047 / 2048 / 2049 and at 80000 (K = 8000): the worst
        |value - float64| over its radius for a_std, m_std, xcorr and peak_corr (<= 1 passes), how many values differ from the
        float32 mirror of the documented summation order (n <= 4099), the lead of the float64 peak over the runner-up against
        twice the largest radius, and whether the lag is the reference's (the fixture's cases).
"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np
import torch

import avlag_ref as R
from ultrafnd_git_amd import temporal

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("avlag_errors.py measures the kernels on a GPU: none found (no CPU fallback)")
out = []
ALL = ("lag_samples", "lag_seconds", "peak_corr", "xcorr", "a_std", "m_std")


def say(s):
    print(s, flush=True)
    out.append(s)


def pair(rng, n, shift):
    base = np.convolve(rng.standard_normal(n + 2 * abs(shift) + 2), [0.25, 0.5, 0.25], "valid")
    p = abs(shift)
    m = (0.6 + 0.25 * base[p:p + n]).astype(np.float32)
    return (1.0 + 0.2 * base[p - shift:p - shift + n] + 0.02 * rng.standard_normal(n)).astype(np.float32), m


cases = {k: v for k, v in R.load_fixture(REPO / "tests" / "golden" / "avlag.npz").items() if v["kind"] in ("regular", "outside")}
rng = np.random.default_rng(78)
for n, K, shift in ((2047, 40, 17), (2048, 40, -33), (2049, 40, 40), (80000, 8000, 5000)):
    x, m = pair(rng, n, shift)
    cases[f"seeded_n{n}"] = {"a": x, "m": m, "sr": 1.0, "max_lag_s": float(K), "seconds": None}

say(f"# av_lag on {torch.cuda.get_device_name(0)}: worst |value - float64| / radius per output (tests/avlag_ref.py: radii); <= 1 passes")
say(f"{'case':16s} {'n':>6s} {'Kc':>5s} {'a_std':>8s} {'m_std':>8s} {'xcorr':>8s} {'peak':>8s} {'radius/n':>9s} {'lead/2r':>9s} {'!= mirror':>10s} {'lag':>10s}")
worst = {k: 0.0 for k in ("a_std", "m_std", "xcorr", "peak_corr")}
for name, c in cases.items():
    K = R.max_lag(c["sr"], c["max_lag_s"])
    w, rad = R.window64(c["a"], c["m"], K), R.radii(c["a"], c["m"], K)
    n, Kc = w["n"], w["Kc"]
    o = {k: v.cpu().numpy()[0] for k, v in
         temporal.av_lag(torch.from_numpy(c["a"])[None].cuda(), torch.from_numpy(c["m"])[None].cuda(), None, None, c["sr"], 25.0, c["max_lag_s"], ALL).items()}
    xc = o["xcorr"][K - Kc:K + Kc + 1]
    frac = {"a_std": float((np.abs(o["a_std"][:n] - w["a_std"]) / rad["a_std"]).max()), "m_std": float((np.abs(o["m_std"][:n] - w["m_std"]) / rad["m_std"]).max()),
            "xcorr": float((np.abs(xc - w["c"]) / rad["c"]).max())}
    j = int(o["lag_samples"]) + Kc
    frac["peak_corr"] = float(abs(float(o["peak_corr"]) - w["c"][j] / n) / rad["peak"][j])
    for k in worst:
        worst[k] = max(worst[k], frac[k])
    if n <= 4099:
        mir = R.mirror(c["a"], c["m"], K)
        diff = sum(int((x.view(np.uint32) != y.view(np.uint32)).sum()) for x, y in ((o["a_std"][:n], mir["a_std"]), (o["m_std"][:n], mir["m_std"]), (xc, mir["c"])))
        diff = str(diff)
    else:
        diff = "-"
    lead = R.margin(w["c"]) / (2.0 * rad["c"].max()) if w["c"].size > 1 else float("inf")
    lag = "-" if c["seconds"] is None else ("reference" if float(o["lag_seconds"]) == c["seconds"] else "DIFFERS")
    say(f"{name:16s} {n:6d} {Kc:5d} {frac['a_std']:8.4f} {frac['m_std']:8.4f} {frac['xcorr']:8.4f} {frac['peak_corr']:8.4f} {rad['c'].max() / n:9.2e} "
        f"{lead:9.1f} {diff:>10s} {lag:>10s}")
say("# worst over all cases: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
