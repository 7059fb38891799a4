"""CPU: tests/motion_ref.py (the NumPy mirror of the reference's OpenCV-less OpticalFlow3DCNN and ChronosGuard) reproduces
tests/golden/motion.npz, minted from the reference's own two classes (tests/golden/make_golden_motion.py): the integer-exact quantities
exactly, the cut scores within one float32 ulp, NaN positions identically, the float statistics within the derived bounds -- which
also shows that the reference's own float32 numbers lie inside every bound, so none is tighter than the yardstick."""
import numpy as np
import pytest

from tests import motion_ref as R


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return R.load_fixture(golden_dir / "motion.npz")


@pytest.fixture(scope="module")
def mirrored(fixture):
    """name -> the mirror's quantities, computed once."""
    out = {}
    for name, ref in fixture.items():
        g = R.gray(ref["frames"])
        h = R.hist32(g)
        out[name] = {"gray": g, "hist": h, "cut64": R.cut_scores64(h), "flows": R.flow_mags(g), "pooled": R.pooled64(g)}
    return out


def test_fixture_holds_the_cases(fixture):
    assert set(fixture) == {"rand7", "down5", "long12", "static6", "cut9", "extremes6", "four4", "three3", "two2", "nine9"}
    assert fixture["down5"]["frames"].shape == (5, 300, 500, 3) and fixture["rand7"]["frames"].shape == (7, 40, 48, 3)
    ex = fixture["extremes6"]["frames"]
    assert (ex[1] == 0).all() and (ex[3] == 255).all()
    for name, ref in fixture.items():
        assert ref["features"].shape == (128,) and ref["pooled"].shape == (77,) and ref["flow256"].shape == (256,) and ref["flow512"].shape == (512,)
        assert ref["cut_scores"].shape == ref["flows"].shape == (len(ref["frames"]) - 1,)


def test_flow_magnitudes_are_exact(fixture, mirrored):
    for name, ref in fixture.items():
        assert np.array_equal(mirrored[name]["flows"], ref["flows"]), name


def test_cut_scores_within_one_ulp(fixture, mirrored):
    unequal = 0
    for name, ref in fixture.items():
        d = R.ulp_distance32(mirrored[name]["cut64"].astype(np.float32), ref["cut_scores"])
        assert d.max() <= 1, (name, d)
        unequal += int((d != 0).sum())
    print("cut scores not bit-equal to the fixture:", unequal)


def test_pooled_counts_maxima_and_nan_positions_are_exact(fixture, mirrored):
    for name, ref in fixture.items():
        p, want = mirrored[name]["pooled"], ref["pooled"].reshape(7, 11)
        assert np.array_equal(np.isnan(p["vector"]), np.isnan(ref["pooled"])), name
        assert np.array_equal(p["bins"].astype(np.float32), want[:, 3:]), name
        assert np.array_equal(p["max"].astype(np.float32), want[:, 2], equal_nan=True), name
        for key in ("flow256", "flow512"):
            dim = ref[key].size
            assert np.array_equal(np.isnan(R.tile_normalise64(p["vector"], dim)), np.isnan(ref[key])), (name, key)
    assert np.isnan(fixture["four4"]["flow256"]).all() and np.isfinite(fixture["down5"]["flow256"]).all()       # 4 frames: NaN; 5: finite
    assert np.isnan(fixture["static6"]["features"]).all() and np.isfinite(fixture["static6"]["tamper"])


def test_reference_float32_statistics_lie_inside_the_bounds(fixture, mirrored):
    """The yardstick itself, held to every bound: the reference's float32 numbers against the float64 evaluation."""
    worst = {}
    def ratio(key, err, bound):
        ok = err <= bound
        assert np.all(ok), (key, err, bound)
        with np.errstate(all="ignore"):
            r = np.nanmax(np.where(bound > 0, err / bound, 0.0))
        worst[key] = max(worst.get(key, 0.0), float(r))
    for name, ref in fixture.items():
        cut, flows = ref["cut_scores"], ref["flows"]
        s64, sb = R.chronos_stats64(cut, flows), R.chronos_bounds(cut, flows)
        assert np.array_equal(np.isnan(s64), np.isnan(ref["stats"])), name
        fin = np.isfinite(s64)
        ratio("chronos stats", np.abs(ref["stats"].astype(np.float64) - s64)[fin], sb[fin])
        if fin.all():
            ratio("chronos vector", np.abs(ref["features"] - R.tile_normalise64(s64, 128)).max(), R.vector_bound(s64, sb, 128))
        assert abs(float(ref["tamper"]) - R.tamper64(ref["stats"].astype(np.float64))) <= 1e-12, name      # float64 Python arithmetic on the float32 statistics
        p = mirrored[name]["pooled"]
        pb = R.pooled_bounds(p)
        fin = np.isfinite(p["vector"])
        ratio("pooled", np.abs(ref["pooled"].astype(np.float64) - p["vector"])[fin], pb[fin])
        if fin.all():
            for key in ("flow256", "flow512"):
                dim = ref[key].size
                ratio(key, np.abs(ref[key] - R.tile_normalise64(p["vector"], dim)).max(), R.vector_bound(p["vector"], pb, dim))
    print("reference float32 vs float64, worst error / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values())


def test_series_are_conditioned_as_the_bounds_assume(fixture):
    for name, ref in fixture.items():
        if name in R.CLIP_NAMES_DEGENERATE:
            continue
        for s in (ref["cut_scores"].astype(np.float64), ref["flows"].astype(np.float64)):
            assert s.std() / s.mean() >= 0.05, name


def test_histogram_table_is_np_histogram_for_all_256_values():
    for v in range(256):
        h, _ = np.histogram(np.array([v], np.uint8), bins=32, range=(0, 255))
        assert h[R.HIST_LUT[v]] == 1 and h.sum() == 1, v
    edges = np.linspace(0, 255, 33)
    assert np.all(np.diff(edges) == R.BIN_WIDTH)


def test_eight_bin_rule_on_edges_and_random_float32():
    rng = np.random.default_rng(5)
    a = np.concatenate([np.arange(9, dtype=np.float32) / np.float32(8), rng.random(200_000, dtype=np.float32),
                        (rng.integers(0, 4000, 5000) / rng.integers(1, 1000, 5000)).astype(np.float32).clip(0, 1)])
    h, _ = np.histogram(a, bins=8, range=(0.0, 1.0))
    assert np.array_equal(h, R.bins8(a))
    for k in range(9):      # the edges one by one: k / 8 opens bin k, and 1.0 closes bin 7
        one = np.array([k / 8], np.float32)
        assert np.array_equal(np.histogram(one, bins=8, range=(0.0, 1.0))[0], R.bins8(one)) and R.bins8(one)[min(k, 7)] == 1


def test_angle_constants():
    for sign, want in R.ANGLES.items():
        fy = np.array([sign * 3.0], np.float32)
        fx = np.zeros(1, np.float32)
        ang = (np.arctan2(fy, fx) + np.pi) / (2 * np.pi)
        assert ang.dtype == np.float32 and ang[0] == np.float32(want), (sign, ang)


def test_integer_luma_formula_is_wrong_on_some_triple():
    """(2989 r + 5870 g + 1140 b) // 10000 is not the float64 expression: a later 'simplification' to integers changes pixels."""
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.arange(0, 256, 5), indexing="ij")
    rgb = np.stack([r, g, b], axis=-1).astype(np.uint8)
    exact = R.luma(rgb)
    integer = ((2989 * r + 5870 * g + 1140 * b) // 10000).astype(np.uint8)
    assert (exact != integer).sum() > 0
    # and the truncation never leaves uint8: the weights sum to 0.9999
    assert exact.max() == 254 and R.luma(np.full((1, 3), 255, np.uint8))[0] == 254


def test_resize_index_rule():
    from math import floor
    for n in (1, 7, 40, 48, 255, 256, 257, 300, 500, 720, 1280):
        assert R.source_index(n).tolist() == [floor(y * n / 256) for y in range(256)], n


def test_chunks_are_array_slicing():
    for pairs in range(0, 40):
        arr = np.arange(pairs)
        want = []
        for level in range(3):
            parts = 2 ** level
            seg = max(1, pairs // parts)
            for p in range(parts):
                want.append(arr[p * seg:(p + 1) * seg] if p < parts - 1 else arr[p * seg:])
        got = R.chunks(pairs)
        assert [arr[lo:hi].tolist() for lo, hi in got] == [w.tolist() for w in want], pairs
        assert any(hi == lo for lo, hi in got) == (pairs < 4), pairs


def test_one_frame_is_all_zeros():
    g = R.gray(np.full((1, 5, 4, 3), 77, np.uint8))
    assert R.flow_mags(g).shape == (0,) and R.pair_sums(g).shape == (0,) and not R.pooled64(g)["vector"].any()
    assert not R.chronos_stats64(np.zeros(0), np.zeros(0)).any() and R.cut_scores64(R.hist32(g)).shape == (0,)


def test_to_uint8_is_per_frame():
    rng = np.random.default_rng(3)
    f = np.stack([rng.random((4, 5, 3)), rng.random((4, 5, 3)) * 300 - 20, np.full((4, 5, 3), 1.0)]).astype(np.float32)
    u = R.to_uint8(f)
    assert np.array_equal(u[0], (f[0] * 255.0).clip(0, 255).astype(np.uint8)) and np.array_equal(u[1], f[1].clip(0, 255).astype(np.uint8))
    assert (u[2] == 255).all()
