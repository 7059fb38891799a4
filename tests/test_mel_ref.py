"""CPU: the float64 restatement of the librosa-branch mel spectrogram in dB (tests/mel_ref.py) against what can be checked without
librosa -- the filterbank against transformers.audio_utils.mel_filter_bank, the STFT against scipy.signal.stft, the exact fmaf
mirror against rational arithmetic -- and its bounds against a table of named mistakes: each mistake, applied to the restatement,
must leave the bounds on at least one named case, so the bounds the device is held to are not vacuous.
Nothing here is verified against librosa itself, and there is no fixture of the reference for this branch (it needs librosa)."""
from fractions import Fraction

import numpy as np
import pytest

import mel_ref as M
from ultrafnd_git_amd import audio


@pytest.fixture(scope="module")
def world():
    clips = M.cases()
    return {"clips": clips, "bounds": {n: M.bounds(x) for n, x in clips.items()}}


def test_filterbank_equals_the_independent_implementation_in_every_value():
    tr = pytest.importorskip("transformers")
    from transformers.audio_utils import mel_filter_bank
    ref = mel_filter_bank(num_frequency_bins=201, num_mel_filters=64, min_frequency=0.0, max_frequency=8000.0, sampling_rate=16000, norm="slaney",
                          mel_scale="slaney")
    assert tr is not None and ref.shape == (201, 64)
    fb = audio.mel_filterbank()
    assert fb["weights"].shape == (64, 201) and fb["weights"].dtype == np.float32
    assert np.array_equal(fb["weights"], ref.T.astype(np.float32))
    mine = M.filterbank()      # the restatement of the tests, written from the formula: the same float32 values, the same supports
    assert np.array_equal(mine.astype(np.float32), fb["weights"]) and np.array_equal(mine != 0, ref.T != 0)
    assert np.abs(mine - ref.T).max() <= 1e-15


def test_filterbank_facts():
    fb = audio.mel_filterbank()
    w, first, count, packed = fb["weights"], fb["first"], fb["count"], fb["packed"]
    assert np.count_nonzero(w) == 388 == len(packed) == int(count.sum()) and np.count_nonzero(packed) == 388
    assert count.min() == 2 and count.max() == 18
    at = 0
    for i in range(64):      # contiguous supports, packed row after row
        row = np.zeros(201, dtype=np.float32)
        row[first[i]:first[i] + count[i]] = packed[at:at + count[i]]
        at += count[i]
        assert np.array_equal(row, w[i]), i
    assert not w[:, 0].any() and not w[:, 200].any()
    assert (first[0], count[0]) == (1, 2) and (first[63], first[63] + count[63] - 1) == (182, 199)
    m = audio.mel_points()
    assert len(m) == 66 and m[0] == 0.0 and abs(m[65] - 8000.0) < 1e-9 and abs(m[1] - 46.4057851) < 5e-8
    assert m[21] < 1000.0 <= m[22]
    assert np.abs(m - M.mel_points()).max() <= 1e-10
    f2, c2 = M.supports(M.filterbank())
    assert np.array_equal(f2, first) and np.array_equal(c2, count)
    assert [audio.mel_frame_count(n) for n in (0, 1, 159, 160, 10240)] == [0, 1, 1, 2, 65] == [M.frame_counts(n)[0] for n in (0, 1, 159, 160, 10240)]


def test_stft_geometry_equals_scipy():
    from scipy.signal import stft
    rng = np.random.default_rng(5)
    for n in (400, 401, 559, 560, 561, 1207, 16000):      # (scipy needs n >= n_fft)
        x = rng.standard_normal(n).astype(np.float32)
        mine = M.stft_mag(x, "A")
        _, _, Z = stft(x.astype(np.float64), window="hann", nperseg=400, noverlap=240, boundary="zeros", padded=False)
        ref = np.abs(Z) * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 400)).sum()
        assert mine.shape == ref.shape == (201, 1 + n // 160)
        assert np.abs(mine - ref).max() <= 1e-10, n


def test_fmaf_mirror_differs_from_the_naive_one_on_a_tie_and_is_exact_on_random_chains():
    # c = 1 + 2^-23 (odd), a b = 2^-24 - 2^-70: the float64 sum is the float32 tie c + 2^-24, which rounds to the even neighbour
    # ABOVE; the exact sum lies below the tie and rounds to c
    a, b, c = np.float32(1.0 + 2.0 ** -23), np.float32(2.0 ** -24 * (1.0 - 2.0 ** -23)), np.float32(1.0 + 2.0 ** -23)
    exact = M.round32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
    assert exact == c and M.fma32(a, b, c) == exact and M.fma32_naive(a, b, c) == np.nextafter(c, np.float32(2)) != exact
    assert M.fma32(-a, b, -c) == -c and M.fma32_naive(-a, b, -c) != -c      # and mirrored in sign
    rng = np.random.default_rng(7)
    n, length = 1000, 12
    w = (rng.random((n, length)) * 10.0 ** rng.integers(-6, 1, (n, length))).astype(np.float32)
    p = (rng.random((n, length)) * 10.0 ** rng.integers(-8, 3, (n, length))).astype(np.float32)
    # a fifth of the chains on a grid of few bits, where ties of the float64 sum actually occur
    w[::5] = (rng.integers(1, 1 << 12, (n // 5, length)) * 2.0 ** -12).astype(np.float32)
    p[::5] = (rng.integers(1, 1 << 13, (n // 5, length)) * 2.0 ** -25).astype(np.float32)
    acc = np.zeros(n, dtype=np.float32)
    for k in range(length):
        acc = M.fma32(w[:, k], p[:, k], acc)
    for i in range(n):
        q = np.float32(0.0)
        for k in range(length):
            q = M.round32(Fraction(float(w[i, k])) * Fraction(float(p[i, k])) + Fraction(float(q)))
        assert q == acc[i], i


def test_the_mirror_of_exact_magnitudes_lies_inside_the_bounds(world):
    """The fp32 chain on the float64 magnitudes rounded once is one admissible device: it must sit inside the power bounds."""
    fb = audio.mel_filterbank()
    for name, x in world["clips"].items():
        S32 = M.stft_mag(x, "A").astype(np.float32)
        P = M.mel_power_mirror(S32, fb["weights"], fb["first"], fb["count"])
        assert M.inside(P, world["bounds"][name]["mel_power"]).all(), name
        T = P.shape[1]
        assert T == M.frame_counts(len(x))[0]


def test_the_restatement_lies_inside_its_own_bounds_and_the_cases_are_what_they_claim(world):
    for name, b in world["bounds"].items():
        assert M.outside_names(b["center"], b) == [], name
    D = {n: b["center"]["mel_db"] for n, b in world["bounds"].items()}
    raw = {n: M.mel_db(x, "no_floor")["mel_db"] for n, x in world["clips"].items()}
    print({n: (float(raw[n].min()), float((raw[n] < -80).mean())) for n in D})
    assert raw["noise"].min() > -80.0      # nothing is floored on white noise
    assert raw["half_silent"].min() < -80.0 and 0.3 < (raw["half_silent"] < -80.0).mean() < 0.7
    assert (raw["tone440"] < -80.0).mean() > 0.5
    q = D["quiet_then_loud"]
    assert q.shape == (64, 130) and q[:, :64].max() < -40.0 and q[:, 128:].max() == 0.0
    assert not D["zeros"].any() and D["zeros"].shape == (64, 26)
    for n in D:
        assert D[n].max() == 0.0 and D[n].min() >= -80.0, n


def test_bounds_on_white_noise_are_a_few_thousandths_of_a_db_wide(world):
    lo, hi = world["bounds"]["noise"]["mel_db"]
    width = hi - lo
    print("white noise: dB interval width min / median / max =", float(width.min()), float(np.median(width)), float(width.max()))
    assert float(np.median(width)) < 0.05
    shifted = {"mel_db": world["bounds"]["noise"]["center"]["mel_db"] + 2.0 ** -8}
    assert M.outside_names(shifted, world["bounds"]["noise"]) == ["mel_db"]
    shifted = {"mel_db": world["bounds"]["noise"]["center"]["mel_db"] - 2.0 ** -8}
    out = ~M.inside(shifted["mel_db"], world["bounds"]["noise"]["mel_db"])
    print("shift by -2^-8: entries outside =", int(out.sum()), "of", out.size)


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_every_named_mistake_leaves_the_bounds_on_some_named_case(world, mistake):
    hit = {}
    for name, x in world["clips"].items():
        out = M.outside_names(M.mel_db(x, mistake), world["bounds"][name])
        if out:
            hit[name] = out
    print(mistake, hit)
    assert hit, mistake
    if mistake in ("no_floor", "floor_before_ref"):      # (these two need a live floor)
        assert "half_silent" in hit or "tone440" in hit, hit
    if mistake == "per_tile_ref":
        assert "quiet_then_loud" in hit, hit
