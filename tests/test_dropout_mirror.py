"""CPU: the host mirror of the kernels' dropout masks (tests/dropout_mirror.py) is Philox4x32-10 and drops at the stated rate."""
import numpy as np
import pytest

from tests import dropout_mirror as D

# Random123 known-answer vectors for philox4x32-10: (counter c0..c3, key k0 k1) -> output
KAT = [((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
        (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
        (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,expect", KAT)
def test_philox_known_answers(ctr, key, expect):
    out = D.philox4x32_10(*ctr, *key)
    assert [int(w) for w in out] == list(expect)


@pytest.mark.parametrize("ctr,key,expect", KAT)
def test_kernel_counter_layout_reaches_the_known_answers(ctr, key, expect):
    """The kernels' mapping: c0 = elem >> 2, c1 = layer, (c2, c3) = step (lo, hi), (k0, k1) = seed (lo, hi); word elem & 3."""
    seed = key[0] | (key[1] << 32)
    step = ctr[2] | (ctr[3] << 32)
    elem = np.array([4 * ctr[0] + q for q in range(4)], dtype=np.uint64)
    got = D.words(seed, step, ctr[1], elem)
    assert [int(w) for w in got] == list(expect)


def test_multiplier_values_and_index_formula():
    """keep <=> float32((word >> 8) / 2^24) >= p; kept elements are scaled by float32 1 / (1 - p); element (r, c) is r * ld + c."""
    seed, step, layer, p = 0x1234_5678_9ABC, 7, D.LAYER_PRE0, 0.1
    m = D.multipliers(seed, step, layer, p, 3, 10, 12)
    w = D.words(seed, step, layer, np.arange(36, dtype=np.uint64)).reshape(3, 12)[:, :10]
    u = (w >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    keep = np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.1))
    assert m.dtype == np.float32
    assert np.array_equal(m, np.where(u >= np.float32(0.1), keep, 0.0).astype(np.float32))
    assert np.array_equal(D.multipliers(seed, step, layer, 0.0, 3, 10, 12), np.ones((3, 10), np.float32))
    # a different tag, step or leading dimension is a different mask
    for other in (D.multipliers(seed, step, D.LAYER_PRE3, p, 3, 10, 12), D.multipliers(seed, step + 1, layer, p, 3, 10, 12),
                  D.multipliers(seed, step, layer, p, 3, 10, 10)):
        assert not np.array_equal(m, other)


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_keep_rate_is_binomial(p):
    """About 10^6 draws of one site: the kept fraction within 5 binomial standard deviations of 1 - p."""
    n_rows, n_cols = 1000, 1024
    m = D.multipliers(99, 3, D.LAYER_FUSE0, p, n_rows, n_cols, n_cols)
    n = m.size
    kept = int((m > 0).sum())
    sd = (n * p * (1 - p)) ** 0.5
    assert abs(kept - n * (1 - p)) <= 5 * sd, (kept, n * (1 - p), sd)
    assert set(np.unique(m).tolist()) == {0.0, float(D.keep_multiplier(p))}
    # the mean multiplier is 1 (inverted dropout), to the same tolerance
    assert abs(float(m.astype(np.float64).mean()) - 1.0) <= 5 * sd / n / (1 - p)
