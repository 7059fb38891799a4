"""CPU: the resampler's host side (ultrafnd_git_amd/audio.py: resample_taps, resampled_length, the device tables) against the
formulas restated in tests/resample_ref.py, the mirror against scipy.signal.upfirdn as an independent formulation, the refusals,
and the ordering of the three qualities on the alias residual.  The measured filter figures are printed here and kept in
profiles/resample_errors.txt (tools/resample_errors.py writes that file)."""
import numpy as np
import pytest
from scipy.signal import upfirdn

import resample_ref as R
from ultrafnd_git_amd import _lib as L
from ultrafnd_git_amd import audio
from ultrafnd_git_amd.audio import resample_taps, resampled_length

CASES = [(o, n, q) for (o, n) in R.PAIRS for q in R.QUALITIES]


@pytest.fixture(scope="module")
def tables():
    return {c: (resample_taps(*c), R.taps_ref(*c)) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_tap_table_equals_the_formulas(tables, case):
    mine, ref = tables[case]
    for key in ("o", "n", "width", "K"):
        assert mine[key] == ref[key], key
    assert np.array_equal(mine["first"], ref["first"]) and np.array_equal(mine["count"], ref["count"])
    assert mine["h"].dtype == np.float32 and mine["h"].shape == (ref["n"], ref["K"])
    # both are float64 evaluations rounded once; two float64 routes to sinc may differ in the last place, which moves an fp32
    # rounding by at most one unit in the last place
    assert (np.abs(mine["h"].astype(np.float64) - ref["h"].astype(np.float64)) <= 2.0 ** -23 * np.abs(ref["h64"])).all()
    assert (mine["h"] != ref["h"]).mean() < 1e-4
    outside = np.ones_like(mine["h"], dtype=bool)
    for p in range(ref["n"]):
        outside[p, ref["first"][p]:ref["first"][p] + ref["count"][p]] = False
    assert not mine["h"][outside].any()


def test_the_issue_table_of_band_lengths():
    want = {44100: (441, 160, 187, 815, 372, 373), 48000: (3, 1, 203, 409, 405, 405), 22050: (441, 320, 94, 629, 186, 187),
            8000: (1, 2, 68, 137, 135, 136)}
    for sr, (o, n, width, K, lo, hi) in want.items():
        t = resample_taps(sr, 16000, "kaiser_best")
        assert (t["o"], t["n"], t["width"], t["K"], int(t["count"].min()), int(t["count"].max())) == (o, n, width, K, lo, hi), sr


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_device_tables_hold_the_same_taps_shifted_per_folded_stride(tables, case):
    t, _ = tables[case]
    G, o, n, K = t["G"], t["o"], t["n"], t["K"]
    dense, pad_rows = R.unpack_device_table(t)
    assert G % 2 == 1 and t["groups"].shape == (-(-G * n // 4), 3) and not pad_rows.any()
    for g in range(G):      # phase g n + p of the super-stride = phase p shifted by g o taps, zeros elsewhere
        want = np.zeros((n, K + (G - 1) * o), dtype=np.float32)
        want[:, g * o:g * o + K] = t["h"]
        assert np.array_equal(dense[g * n:(g + 1) * n], want), g
    lo, cnt, off = t["groups"].T
    assert not (lo % 8).any() and not (cnt % 8).any() and (lo >= 0).all()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)[:-1]])) and off[-1] + cnt[-1] == t["table"].shape[0]
    assert t["kc"] % 8 == 0 and t["kc"] * t["nchunks"] >= int((lo + cnt).max())
    assert 1 <= t["qt"] <= L.RESAMPLE_OUT_TILE and (t["qt"] - 1) * G * o + t["kc"] <= L.RESAMPLE_LDS_FLOATS
    assert t["out_tile"] == t["qt"] * G * n


def test_long_filters_are_chunked_within_the_lds_budget():
    t = resample_taps(1024000, 1000, "kaiser_best")      # o = 1024, n = 1: 138321 taps per phase
    assert t["o"] == 1024 and t["n"] == 1 and t["nchunks"] > 1 and t["qt"] < L.RESAMPLE_OUT_TILE
    assert (t["qt"] - 1) * t["G"] * t["o"] + t["kc"] <= L.RESAMPLE_LDS_FLOATS and t["kc"] * t["nchunks"] >= int((t["first"] + t["count"]).max())
    dense, _ = R.unpack_device_table(t)
    assert np.array_equal(dense[0], t["h"][0])


def test_ratio_one_is_the_one_tap_filter():
    t = resample_taps(16000, 16000, "hann")
    assert (t["o"], t["n"], t["width"], t["K"]) == (1, 1, 0, 1) and t["h"].tolist() == [[1.0]]
    assert t["first"].tolist() == [0] and t["count"].tolist() == [1]
    assert resample_taps(44100, 44100)["h"].tolist() == [[1.0]]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_mirror_equals_upfirdn_of_the_interleaved_prototype(tables, case):
    _, ref = tables[case]
    rng = np.random.default_rng(1)
    x = rng.standard_normal(3 * ref["o"] + 7).astype(np.float32)
    y, _ = R.resample_ref(x, ref)
    g, shift = R.upfirdn_prototype(ref)
    u = upfirdn(g, x.astype(np.float64), up=ref["n"], down=1)
    yy = u[shift::ref["o"]][:len(y)]
    assert len(yy) == len(y) == R.resampled_length_ref(len(x), ref["o"], ref["n"])
    assert np.abs(y - yy).max() <= 1e-12 * np.abs(yy).max()


def test_chain_mirror_stays_inside_the_bound_of_the_float64_mirror(tables):
    rng = np.random.default_rng(2)
    for case in ((44100, 16000, "kaiser_best"), (8000, 16000, "hann"), (16000, 44100, "kaiser_fast")):
        _, ref = tables[case]
        x = (0.1 * rng.standard_normal(1200)).astype(np.float32)
        y, bound = R.resample_ref(x, ref)
        c = R.resample_chain_f32(x, ref)
        assert (np.abs(c.astype(np.float64) - y) <= bound).all(), case


def test_resampled_length_at_the_edges():
    for orig, new in R.PAIRS + ((16000, 16000),):
        t = resample_taps(orig, new, "hann")
        o, n = t["o"], t["n"]
        for length in (0, 1, o - 1, o, o + 1, 7 * o, 7 * o + 1):
            if length < 0:
                continue
            want = int(np.ceil(n * length / o)) if length else 0
            assert resampled_length(length, orig, new) == want == R.resampled_length_ref(length, o, n), (orig, new, length)
    assert resampled_length(0, 44100) == 0 and resampled_length(441, 44100) == 160 and resampled_length(442, 44100) == 161
    assert resampled_length(1 << 30, 8000, 16000) == 1 << 31      # (host integers: no 32-bit wrap)


def test_every_refusal_names_its_limit():
    for bad in (0, -16000, 44100.5, "44100", None, True):
        with pytest.raises(ValueError, match="positive integer"):
            resample_taps(bad, 16000)
        with pytest.raises(ValueError, match="positive integer"):
            resampled_length(10, 16000, bad)
    with pytest.raises(ValueError, match=str(L.RESAMPLE_MAX_RATIO_TERM)):
        resample_taps(44101, 16000)      # coprime: o = 44101
    with pytest.raises(ValueError, match=r"1025/1024.*above 1024"):
        resample_taps(1025, 1024)
    with pytest.raises(ValueError, match=r"1/1025.*above 1024"):
        resample_taps(1, 1025)
    assert resample_taps(1024, 1023, "hann")["o"] == 1024      # the limit itself is accepted
    with pytest.raises(ValueError, match="kaiser_best.*kaiser_fast.*hann"):
        resample_taps(44100, 16000, "sinc_best")
    with pytest.raises(ValueError, match="at least 0"):
        resampled_length(-1, 44100)
    assert L.RESAMPLE_MAX_RATIO_TERM == 1024 and L.RESAMPLE_OUT_TILE == 64


def test_constants_mirror_the_header():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parents[1] / "include" / "ultrafnd_hip.h").read_text()
    for name, val in (("OUT_TILE", L.RESAMPLE_OUT_TILE), ("LDS_FLOATS", L.RESAMPLE_LDS_FLOATS), ("MAX_RATIO_TERM", L.RESAMPLE_MAX_RATIO_TERM),
                      ("F32", L.RESAMPLE_F32), ("I16", L.RESAMPLE_I16)):
        assert int(re.search(rf"#define UFND_RESAMPLE_{name} (\d+)", text).group(1)) == val, name


def filter_figures():
    """Per (rate -> 16 kHz, quality): worst |phase DC sum - 1|, gains of 1 kHz and 3 kHz tones, residual of a tone 2 kHz above the
    new Nyquist (skipped where the source cannot carry it), all on the float64 mirror."""
    rows = []
    for sr in R.PAIRS_TO_16K:
        for q in R.QUALITIES:
            ref = R.taps_ref(sr, 16000, q)
            dc = float(np.abs(ref["h"].astype(np.float64).sum(axis=1) - 1.0).max())
            alias_f = 0.5 * min(sr, 16000) + 2000.0
            alias = R.tone_gain(ref, sr, alias_f) if alias_f < sr / 2 else None
            rows.append({"sr": sr, "quality": q, "dc": dc, "g1k": R.tone_gain(ref, sr, 1000.0), "g3k": R.tone_gain(ref, sr, 3000.0), "alias": alias})
    return rows


def test_quality_ordering_on_the_alias_residual():
    rows = filter_figures()
    for r in rows:
        print(r)
    for sr in R.PAIRS_TO_16K:
        a = {r["quality"]: r["alias"] for r in rows if r["sr"] == sr}
        if a["hann"] is None:
            continue
        assert a["kaiser_best"] <= a["kaiser_fast"] <= a["hann"], (sr, a)
    assert any(r["alias"] is not None for r in rows)
