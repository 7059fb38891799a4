"""CPU: the float64 restatement of the librosa branches (tests/librosa_ref.py) against what can be checked without librosa -- both STFT
geometries against scipy.signal.stft, the band table of spectral_contrast -- and the bounds against a table of named mistakes: each
mistake, applied to the restatement, must leave the bounds on at least one case, so the bounds the device is held to are not vacuous.
Nothing here is verified against librosa itself, and there is no fixture of the reference for this branch (it needs librosa)."""
import numpy as np
import pytest

import librosa_ref as R
from ultrafnd_git_amd import audio

GEOMETRY = audio.DESC_GEOMETRY      # n_fft: hop of the two STFTs the device path is built for


@pytest.fixture(scope="module")
def world():
    clips = R.cases()
    return {"clips": clips, "bounds": {n: R.bounds(x) for n, x in clips.items()}}


@pytest.mark.parametrize("which", ["A", "B"])
def test_stft_geometry_equals_scipy(which):
    from scipy.signal import stft
    n_fft, hop = R.GEOMETRY[which]
    rng = np.random.default_rng(5)
    for n in (n_fft, n_fft + 1, n_fft + hop - 1, n_fft + hop, n_fft + hop + 1, n_fft + 5 * hop + 7, 6000):      # (scipy needs n >= n_fft)
        x = rng.standard_normal(n).astype(np.float32)
        mine = R.stft_mag(x, which)
        _, _, Z = stft(x.astype(np.float64), window="hann", nperseg=n_fft, noverlap=n_fft - hop, boundary="zeros", padded=False)
        ref = np.abs(Z) * R.window(n_fft).sum()
        assert mine.shape == ref.shape == (n_fft // 2 + 1, 1 + n // hop)
        assert np.abs(mine - ref).max() <= 1e-10, (which, n)


def test_the_restatement_and_the_package_agree_on_geometry_and_outputs():
    assert {n_fft: hop for n_fft, hop in R.GEOMETRY.values()} == GEOMETRY
    assert len(R.DESCRIPTORS) == audio.N_DESCRIPTORS and len(R.band_table()) == audio.N_CONTRAST_BANDS
    for n in (0, 1, 159, 160, 511, 512, 10240):
        assert R.frame_counts(n) == audio.desc_frame_counts(n)
    assert set(R.CHECKED) | {"features"} == set(audio.DESC_OUTPUTS)


def test_window_is_the_periodic_hann_window():
    from scipy.signal import get_window
    for n_fft in (400, 2048):
        assert np.abs(R.window(n_fft) - get_window("hann", n_fft, fftbins=True)).max() <= 1e-15


def test_band_table_is_reproduced():
    want = [((0, 5), 5, 1), ((4, 10), 6, 1), ((9, 20), 11, 1), ((19, 40), 21, 1), ((39, 80), 41, 1), ((79, 160), 81, 2), ((159, 200), 42, 1)]
    for k, ((rows, idx), ((first, last), used, widx)) in enumerate(zip(R.band_table(), want)):
        masked_last = rows[-1] + (1 if k < 6 else 0)
        assert (rows[0], masked_last, len(rows), idx) == (first, last, used, widx), k
        assert np.array_equal(rows, np.arange(rows[0], rows[0] + len(rows))), k


def test_the_restatement_lies_inside_its_own_bounds(world):
    for name, b in world["bounds"].items():
        assert R.outside_names(b["center"], b) == [], name
        lo, hi = b["rolloff_bins"]
        k = b["center"]["rolloff"] / (R.SR / 2048.0)
        assert ((k >= lo) & (k <= hi)).all(), name


def test_bounds_on_white_noise_are_tight(world):
    """On white noise the chain bound is a few 1e-3 of a band's minimum: the contrast interval is a fraction of a dB wide and the
    rolloff's possible set a few bins."""
    b = world["bounds"]["noise4000"]
    lo, hi = b["contrast"]
    assert float((hi - lo).max()) < 1.0
    kmin, kmax = b["rolloff_bins"]
    assert int((kmax - kmin).max()) <= 4
    # the descriptors that are sums over many entries stay within 1 % (the minimum of |S| and the two small standard deviations
    # are a few per cent wide: the absolute bound d_t against a small value)
    d, big = b["descriptors"], [0, 1, 2, 4, 6, 8, 9, 10]
    assert ((d[1] - d[0])[big] <= 0.01 * np.abs(b["center"]["descriptors"][big])).all()


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_named_mistake_leaves_the_bounds_on_some_case(world, mistake):
    hit = {}
    for name, x in world["clips"].items():
        out = R.outside_names(R.describe(x, mistake), world["bounds"][name])
        if out:
            hit[name] = out
    print(mistake, hit)
    assert hit, mistake
    white = [n for n in hit if n.startswith("noise")]
    if mistake not in ("no_clip", "rolloff_le"):      # (those two need silence: a live 80 dB clip, a running sum equal to its threshold)
        assert white, (mistake, hit)
