"""CPU: the NumPy mirror tests/forgery_ref.py against libjpeg and against the reference's own numbers (tests/golden/forgery.npz, minted by
tests/golden/make_golden_forgery.py from the reference's DeepForgeryDetector and FaceWarpAnalyzer).

  round trip   the mirror's integer pipeline == Pillow's libjpeg encode + decode in every byte, and == the planes the fixture stores
  features     the mirror's float64 vectors and scores against the reference's float32 ones, under the bounds derived in the mirror
  table        every case and setting is in the fixture, every bound positive and finite
The GPU tests (tests/test_gpu_forgery.py) hold the device to the same mirror, so this file is what ties them to libjpeg and the reference."""
import numpy as np
import pytest

from tests import forgery_cases as C
from tests import forgery_ref as R


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return R.load_fixture(golden_dir / "forgery.npz")


@pytest.fixture(scope="module")
def analysed(fixture):
    """(clip, setting, dim) -> the mirror's results for the clip's middle frame (computed once, shared, never modified)."""
    out = {}
    for name, ref in fixture.items():
        img = R.middle_frame(ref["frames"])
        for setting, qs in C.SETTINGS.items():
            for dim in C.DIMS:
                out[name, setting, dim] = R.analyse(img, dim=dim, jpeg=False) if qs is None else R.analyse(img, quality=qs[0], scale=qs[1], dim=dim)
    return out


@pytest.mark.parametrize("quality", R.QUALITIES)
def test_round_trip_equals_libjpeg_in_every_byte(quality):
    pytest.importorskip("PIL")
    for name, img in C.full_images().items():
        differ = int((R.roundtrip(img, quality) != R.pillow_roundtrip(img, quality)).sum())
        print(f"round trip {name} quality {quality}: bytes that differ from libjpeg's: {differ}")
        assert differ == 0, (name, quality)


def test_round_trip_of_resized_small_sources_equals_libjpeg():
    pytest.importorskip("PIL")
    for name, clip in C.clips().items():
        rgb = R.resize_rgb(R.middle_frame(clip))
        for quality in (1, 85):
            assert np.array_equal(R.roundtrip(rgb, quality), R.pillow_roundtrip(rgb, quality)), (name, quality)


def test_round_trip_equals_the_fixtures_planes(fixture):
    seen = 0
    for name, quality in C.PLANES.items():
        rgb = R.resize_rgb(R.middle_frame(fixture[name]["frames"]))
        want = fixture[name][f"rec{quality}"]
        assert want.shape == (256, 256, 3) and want.dtype == np.uint8
        assert np.array_equal(R.roundtrip(rgb, quality), want), (name, quality)
        assert not np.array_equal(want, rgb), name          # a real round trip, not the copy
        seen += 1
    assert seen == 3


def test_quantisation_tables():
    assert np.array_equal(R.qtables(50), np.stack([R.K1, R.K2]))
    assert (R.qtables(100) == 1).all() and R.qtables(1).max() == 255 and R.qtables(1).min() == 255
    assert R.qtables(85)[0, 0] == 5 and R.qtables(85)[1, 63] == 30
    from ultrafnd_git_amd import video
    for q in range(1, 101):
        assert bytes(video.jpeg_qtables(q)) == bytes(R.qtables(q).astype(np.uint8).ravel()), q


def test_vectors_against_the_reference(fixture, analysed):
    for (name, setting, dim), a in analysed.items():
        want = fixture[name][f"{setting}/vec{dim}"]
        err = np.abs(a["features"] - want.astype(np.float64)).max()
        bound = R.vector_bound(a["stats"], a["lbp"], dim)
        print(f"FORGERY_REF {name} {setting} vec{dim} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, setting, dim, err, bound)
    # without a round trip the map is zero and the vector the same constant for every image
    const = {tuple(fixture[n]["none/vec256"]) for n in fixture}
    assert len(const) == 1 and analysed["noise5", "none", 256]["stats"].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert len({tuple(fixture[n]["q85s1/vec256"]) for n in fixture}) >= 5


def test_scores_against_the_reference(fixture, analysed):
    for name, ref in fixture.items():
        for setting in ("none", "q85s1", "q1s10"):            # the score's own map is quality 85, scale 1 whatever the detector's is
            a = analysed[name, setting, 256]
            want = float(ref[("none" if setting == "none" else "q85s1") + "/score"])
            err, bound = abs(a["score"] - want), R.score_bound(a["grad"])
            print(f"FORGERY_REF {name} {setting} score err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (name, setting, err, bound)
    flat = analysed["static2", "q85s1", 256]
    assert flat["grad"].tolist() == [0.0, 0.0] and flat["score"] == 0.5 * flat["ela85_mean"] / 255.0


def test_every_case_is_covered_and_every_bound_is_positive_and_finite(fixture, analysed):
    assert set(fixture) == set(C.clips()) and len(fixture) == 7
    for name, clip in C.clips().items():
        assert np.array_equal(fixture[name]["frames"], clip), name
        for setting in C.SETTINGS:
            for dim in C.DIMS:
                assert fixture[name][f"{setting}/vec{dim}"].shape == (dim,), (name, setting, dim)
    assert set(C.PLANES) <= set(fixture) and set(C.PLANES.values()) <= set(R.QUALITIES)
    assert {qs[0] for qs in C.SETTINGS.values() if qs} == set(R.QUALITIES)
    assert {qs[1] for qs in C.SETTINGS.values() if qs} == {1.0, 0.5, 10.0}
    for key, a in analysed.items():
        vb, sb, gb = R.vector_bound(a["stats"], a["lbp"], key[2]), R.score_bound(a["grad"]), R.grad_bounds(a["grad"])
        assert np.isfinite(vb) and 0 < vb < 1e-4, (key, vb)
        assert np.isfinite(sb) and 0 < sb < 1e-4, (key, sb)
        assert np.isfinite(gb).all() and (gb >= 0).all() and ((gb > 0).all() or a["grad"][0] == 0), (key, gb)
    # the cases exercise what they are there for
    assert analysed["sat1", "q1s10", 256]["stats"][2] == 255 and analysed["noise5", "q50s05", 256]["ela"].max() < 128
    assert analysed["wide2", "q85s1", 256]["rgb"].shape == (256, 256, 3) and len(np.unique(analysed["one1", "q85s1", 256]["rgb"].reshape(-1, 3), axis=0)) == 1
