#!/usr/bin/env python3
"""Mint tests/golden/avlag.npz from the REAL reference's two estimate_av_lag functions: TemporalSyncNet
(src/core_blocks/temporal_blocks.py:176-223) and ChronosGuard (src/models/chronos_guard.py:175-196).

Needs a checkout of the reference project (it is not part of this repository and never travels with it):

    python tests/golden/make_golden_avlag.py <path to the reference checkout>

Every case is a pair of float32 series, the call's sr / fps / max_lag_s and the seconds the reference returned (both functions
must agree, asserted).  Data only.  A regular case is a smoothed seeded noise series on an offset (`m`) and a noisy copy of it moved by
`shift` samples (`a[i + shift] = m[i]`, so the reference answers +shift / sr while the shift is inside the window; asserted from
16 samples up), both rounded to multiples of 2^-10 so that the file compresses.  The cases:
  n in 3, 4, 5, 16, 63, 64, 65, 125, 257, 1000, 4099, 20000; shifts +, -, 0; +-(K - 1) (n = 1000 at sr = 100 and n = 20000 at
  sr = 16000) and one outside the window (n = 20000, sr = 16000, shift 9000 > K = 8000, with a weaker copy at lag -1234, which is
  what the reference then returns); sr = 25 and sr = 100 with K >= n - 1; K = 0;
  len_a != len_m, both ways; an all-zero a (twice); the constant 0.5 at n = 16.
For every non-degenerate case (n >= 4, more than one lag, a not constant) the generator asserts that the float64 peak of
tests/avlag_ref.py's restatement leads the runner-up by more than twice the largest radius of the device's bound, and that the
restatement's argmax is what the reference returned.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SEED = 2027

# name, len_a, len_m, sr, max_lag_s, shift, kind
CASES = (
    ("n3", 3, 3, 16000.0, 0.5, 0, "short"),
    ("n4", 4, 4, 16000.0, 0.5, 0, "regular"),
    ("n5_sr25", 5, 5, 25.0, 0.5, 1, "regular"),
    ("n16_sr100", 16, 16, 100.0, 0.5, -2, "regular"),
    ("n63", 63, 63, 16000.0, 0.5, 5, "regular"),
    ("n64", 64, 64, 16000.0, 0.5, -7, "regular"),
    ("n64_k0", 64, 64, 16000.0, 0.0, 3, "regular"),
    ("n65", 65, 65, 16000.0, 0.5, 0, "regular"),
    ("n125_sr100", 125, 125, 100.0, 0.5, 9, "regular"),
    ("n125_sr25", 125, 125, 25.0, 0.5, -11, "regular"),
    ("n257", 257, 257, 16000.0, 0.5, -40, "regular"),
    ("la300_lm257", 300, 257, 100.0, 0.5, 13, "regular"),
    ("la125_lm200", 125, 200, 100.0, 0.5, -6, "regular"),
    ("n1000_plus", 1000, 1000, 100.0, 0.5, 49, "regular"),
    ("n1000_minus", 1000, 1000, 100.0, 0.5, -49, "regular"),
    ("n4099", 4099, 4099, 16000.0, 0.5, -100, "regular"),
    ("n20000_edge", 20000, 20000, 16000.0, 0.5, 7999, "regular"),
    ("n20000_outside", 20000, 20000, 16000.0, 0.5, 9000, "outside"),
    ("zero_a_n16", 16, 16, 16000.0, 0.5, 0, "zero_a"),
    ("zero_a_n125", 125, 125, 100.0, 0.5, 0, "zero_a"),
    ("const_half_n16", 16, 16, 16000.0, 0.5, 0, "const_half"),
)


ECHO = -1234      # the `outside` case: a weaker copy at this lag, so that the peak INSIDE the window is a planted one too


def series(rng, la: int, lm: int, shift: int, echo: int = None):
    """m = 0.6 + smoothed noise, a = 1.0 + 0.8 (the same series moved by `shift`) + noise (+ half as much of it moved by `echo`); multiples
    of 2^-10."""
    n = max(la, lm)
    pad = max(abs(shift), abs(echo or 0)) + 8
    raw = rng.standard_normal(n + 2 * pad + 2)
    base = (raw[:-2] + 2.0 * raw[1:-1] + raw[2:]) / 4.0 if n >= 8 else raw[:-2]      # (a series of 4 or 5 samples is left rough)
    m = 0.6 + 0.25 * base[pad:pad + lm]
    a = 1.0 + 0.2 * base[pad - shift:pad - shift + la] + 0.02 * rng.standard_normal(la)
    if echo is not None:
        a = a + 0.1 * base[pad - echo:pad - echo + la]
    q = lambda v: (np.round(v * 1024.0) / 1024.0).astype(np.float32)
    return q(a), q(m)


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "src" / "core_blocks" / "temporal_blocks.py").is_file():
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.modules["cv2"] = None
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ref))
    sys.path.insert(0, str(HERE.parent))
    import src.core_blocks.temporal_blocks as tb
    import src.models.chronos_guard as cg
    import avlag_ref as R

    rng = np.random.default_rng(SEED)
    store = {"names": []}
    for name, la, lm, sr, max_lag_s, shift, kind in CASES:
        if kind == "zero_a":
            a, m = np.zeros(la, np.float32), series(rng, la, lm, 0)[1]
        elif kind == "const_half":
            a, m = np.full(la, 0.5, np.float32), series(rng, la, lm, 0)[1]
        else:
            a, m = series(rng, la, lm, shift, ECHO if kind == "outside" else None)
        sec = tb.TemporalSyncNet.estimate_av_lag(a, m, sr=sr, fps=25.0, max_lag_s=max_lag_s)
        sec_cg = cg.ChronosGuard.estimate_av_lag(a, m, sr=sr, fps=25.0, max_lag_s=max_lag_s)
        assert isinstance(sec, float) and sec == sec_cg, (name, sec, sec_cg)
        K = R.max_lag(sr, max_lag_s)
        n = min(la, lm)
        note = ""
        if kind in ("regular", "outside") and n >= 4:
            w, rad = R.window64(a, m, K), R.radii(a, m, K)
            assert R.lag64(a, m, sr, 25.0, max_lag_s) == sec, (name, R.lag64(a, m, sr, 25.0, max_lag_s), sec)
            if abs(shift) <= w["Kc"] and n >= 16:      # (4 or 5 samples carry no reliable peak: whatever the reference returns is the answer)
                assert sec == shift / sr, (name, sec, shift / sr)
            if kind == "outside":
                assert abs(shift) > w["Kc"] and sec == ECHO / sr, (name, sec)
            if w["c"].size > 1:
                lead, r = R.margin(w["c"]), float(rad["c"].max())
                assert lead > 2.0 * r, (name, lead, r)
                note = f"lead {lead / n:.4f} n, radius {r / n:.2e} n"
        elif n >= 4:      # a standardises to zeros: every c[k] is 0 and the first lag of the window wins
            assert sec == -min(K, n - 1) / sr, (name, sec)
        else:
            assert sec == 0.0, (name, sec)
        store["names"].append(name)
        for key, val in (("a", a), ("m", m), ("sr", np.float64(sr)), ("fps", np.float64(25.0)), ("max_lag_s", np.float64(max_lag_s)),
                         ("seconds", np.float64(sec)), ("shift", np.int64(shift)), ("kind", np.array(kind))):
            store[f"{name}/{key}"] = val
        print(f"{name:16s} n={n:6d} K={K:5d} shift={shift:6d} seconds={sec!r} {note}", flush=True)
    store["names"] = np.array(store["names"])
    path = HERE / "avlag.npz"
    np.savez_compressed(path, **store)
    assert path.stat().st_size < 400_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
