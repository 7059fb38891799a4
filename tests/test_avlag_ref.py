"""CPU: the checker of the A/V lag kernels (tests/avlag_ref.py) against the reference's own answers (tests/golden/avlag.npz, minted
from the reference's two estimate_av_lag functions by tests/golden/make_golden_avlag.py) and against independent arithmetic: the
float64 window against scipy.signal.correlate, the fp32 mirror against a scalar restatement of the documented order and against the
float64 window at the radii, and the named mistakes, each of which leaves the fixture or the radii on some case."""
from pathlib import Path

import numpy as np
import pytest

import avlag_ref as R
from mel_ref import fma32

FIXTURE = Path(__file__).resolve().parent / "golden" / "avlag.npz"


@pytest.fixture(scope="module")
def cases():
    return R.load_fixture(FIXTURE)


def _K(c):
    return R.max_lag(c["sr"], c["max_lag_s"])


def test_the_fixture_holds_the_cases_the_checks_rest_on(cases):
    n = {min(c["a"].size, c["m"].size) for c in cases.values()}
    assert {3, 4, 5, 16, 63, 64, 65, 125, 257, 1000, 4099, 20000} <= n
    assert FIXTURE.stat().st_size < 400_000
    reg = [c for c in cases.values() if c["kind"] == "regular"]
    assert any(c["shift"] > 0 for c in reg) and any(c["shift"] < 0 for c in reg) and any(c["shift"] == 0 for c in reg)
    assert any(abs(c["shift"]) == _K(c) - 1 and c["a"].size == 20000 and c["sr"] == 16000.0 for c in reg)
    assert {c["shift"] for c in reg if c["a"].size == 1000} == {49, -49} and all(_K(c) == 50 for c in reg if c["a"].size == 1000)
    out = cases["n20000_outside"]
    assert out["shift"] > _K(out) and out["sr"] == 16000.0 and out["a"].size == 20000
    assert any(c["sr"] == 25.0 and _K(c) >= c["a"].size - 1 for c in reg) and any(c["sr"] == 100.0 and _K(c) >= c["a"].size - 1 for c in reg)
    assert any(_K(c) == 0 for c in reg) and any(c["a"].size > c["m"].size for c in reg) and any(c["a"].size < c["m"].size for c in reg)
    assert not cases["zero_a_n16"]["a"].any() and (cases["const_half_n16"]["a"] == 0.5).all() and cases["const_half_n16"]["a"].size == 16
    assert cases["zero_a_n16"]["seconds"] == -15 / 16000.0 == cases["const_half_n16"]["seconds"] and cases["n3"]["seconds"] == 0.0


def test_the_restatement_returns_the_reference_s_seconds_in_every_case(cases):
    for name, c in cases.items():
        assert R.lag64(c["a"], c["m"], c["sr"], c["fps"], c["max_lag_s"]) == c["seconds"], name


def test_the_window_is_scipy_s_correlation_of_the_standardised_signals(cases):
    from scipy.signal import correlate
    for name, c in cases.items():
        w = R.window64(c["a"], c["m"], _K(c))
        if w is None:
            continue
        n, Kc = w["n"], w["Kc"]
        a, m = c["a"][:n].astype(np.float64), c["m"][:n].astype(np.float64)
        ah, mh = (a - a.mean()) / (a.std() + 1e-9), (m - m.mean()) / (m.std() + 1e-9)
        full = correlate(ah, mh, mode="full", method="direct")      # index n - 1 + k is lag k
        want = full[n - 1 - Kc:n + Kc]
        assert w["c"].shape == want.shape == (2 * Kc + 1,)
        assert np.abs(w["c"] - want).max() <= 1e-10 * (1.0 + np.abs(want).max()), name
        # the sign convention, spelled out at one lag: c[k] = sum_i ahat[i + k] mhat[i]
        k = min(2, Kc)
        assert abs(w["c"][Kc + k] - float(np.dot(ah[k:], mh[:n - k]))) <= 1e-10 * n, name


def test_margins_and_radii_of_the_fixture(cases):
    """The float64 peak leads the runner-up by more than twice the largest radius, which stays below 1e-3 n."""
    for name, c in cases.items():
        if c["kind"] not in ("regular", "outside") or _K(c) == 0:
            continue
        w, rad = R.window64(c["a"], c["m"], _K(c)), R.radii(c["a"], c["m"], _K(c))
        r = float(rad["c"].max())
        assert R.margin(w["c"]) > 2.0 * r and r < 1e-3 * w["n"], (name, R.margin(w["c"]), r)
        assert R.possible_lags(w["c"], rad["c"], w["Kc"]).tolist() == [round(c["seconds"] * c["sr"])], name
        assert rad["a_std"].max() < 1e-5 and rad["m_std"].max() < 1e-5, name


def test_fma32_chain_and_segment_fold_of_the_mirror_against_a_scalar_restatement(monkeypatch):
    """corr32 with segments of 8: the same bits as the order written out sample by sample."""
    monkeypatch.setattr(R, "SEG", 8)
    rng = np.random.default_rng(5)
    for n, K in ((21, 6), (16, 40), (9, 0)):
        ah, mh = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        got = R.corr32(ah, mh, K)
        Kc = min(K, n - 1)
        for k in range(-Kc, Kc + 1):
            c = None
            for s0 in range(0, n, 8):
                acc = np.float32(0.0)
                for i in range(s0, min(s0 + 8, n)):
                    if 0 <= i + k < n:
                        acc = fma32(ah[i + k], mh[i], acc)[()]
                c = acc if c is None else np.float32(c + acc)
            assert got[k + Kc].view(np.uint32) == np.float32(c + np.float32(0.0)).view(np.uint32), (n, K, k)


def test_the_mirror_lies_inside_the_radii_and_returns_the_fixture_s_lag(cases):
    for name, c in cases.items():
        n = min(c["a"].size, c["m"].size)
        if n > 1000:
            continue
        K = _K(c)
        mir = R.mirror(c["a"], c["m"], K)
        if n < 4:
            assert mir is None
            continue
        assert mir["lag"] / c["sr"] == c["seconds"], name
        if c["kind"] != "regular":      # a constant row: exact zeros (the radius of a vanishing std means nothing)
            assert not mir["a_std"].any() and not mir["c"].any() and mir["lag"] == -mir["Kc"], name
            continue
        w, rad = R.window64(c["a"], c["m"], K), R.radii(c["a"], c["m"], K)
        for k in ("a_std", "m_std", "c"):
            assert (np.abs(mir[k].astype(np.float64) - w[k]) <= rad[k]).all(), (name, k)
        j = mir["lag"] + mir["Kc"]
        assert abs(float(mir["peak"]) - w["c"][j] / n) <= rad["peak"][j], name


def test_statistics_mirror_sums_in_the_documented_order():
    """More than one round of the 1024 threads and a ragged last round: the fold is the one written out here."""
    rng = np.random.default_rng(6)
    v = rng.standard_normal(2500)
    part = [0.0] * 1024
    for i, x in enumerate(v):      # ascending i: thread i % 1024 takes it
        part[i % 1024] = part[i % 1024] + float(x)
    o = 512
    while o:
        for t in range(o):
            part[t] = part[t] + part[t + o]
        o //= 2
    assert R._block_sum(v) == part[0]


def test_every_named_mistake_leaves_the_fixture_or_the_radii(cases):
    caught = {}
    for mistake in R.MISTAKES:
        hits = []
        for name, c in cases.items():
            if R.lag64(c["a"], c["m"], c["sr"], c["fps"], c["max_lag_s"], mistake) != c["seconds"]:
                hits.append((name, "lag"))
            if c["kind"] == "regular":
                K = _K(c)
                w, bad, rad = R.window64(c["a"], c["m"], K), R.window64(c["a"], c["m"], int(c["max_lag_s"] * (c["fps"] if mistake == "k_from_fps" else c["sr"])),
                                                                        mistake), R.radii(c["a"], c["m"], K)
                n = w["n"]
                if bad["a_std"].size != n or (np.abs(bad["a_std"] - w["a_std"]) > rad["a_std"]).any():
                    hits.append((name, "a_std"))
                j, jb = int(np.argmax(w["c"])), int(np.argmax(bad["c"]))
                if abs(bad["c"][jb] / bad["n"] - w["c"][j] / n) > rad["peak"][j]:
                    hits.append((name, "peak_corr"))
        caught[mistake] = hits
        assert hits, mistake
    kinds = lambda m: {k for _, k in caught[m]}
    for m in ("sign_flipped", "swapped", "centre_off_by_one", "window_not_clamped", "ties_highest", "no_mean_removal", "k_from_fps"):
        assert "lag" in kinds(m), (m, caught[m])
    assert kinds("ddof1") & {"a_std", "peak_corr"} and "lag" not in kinds("ddof1")      # the lag is scale-invariant
    assert kinds("longer_input") and {n for n, _ in caught["longer_input"]} <= {"la300_lm257", "la125_lm200"}
    assert {n for n, _ in caught["window_not_clamped"]} >= {"zero_a_n16"} and {n for n, _ in caught["ties_highest"]} >= {"zero_a_n16", "zero_a_n125"}
