"""GPU: ultrafnd_git_amd/video.py (csrc/motion.hip) against the NumPy mirror tests/motion_ref.py and the fixture minted from the
reference's own OpticalFlow3DCNN and ChronosGuard (tests/golden/motion.npz; tests/test_motion_ref.py holds the mirror to it on the CPU).

  exact        gray planes, flow magnitudes, the pyramid's 8-bin counts and chunk maxima, NaN positions: bit for bit
  cut scores   within one float32 ulp of the float64 per-bin evaluation (the count of unequal values is printed; zero is expected)
  statistics   ChronosGuard's mean / std / correlation, the chunks' mean and std of m, both normalised vectors, cache_visual: against the
               mirror's float64 evaluation on the device's own per-pair series and gray planes, under the bounds derived in
               tests/motion_ref.py (bounds of the reference's float32 arithmetic; the device evaluates in double and rounds once).
               Every figure is printed before it is asserted (MOTION_ERR lines: tools/motion_errors.py collects them).
  bits         alone = in a batch = rerun = replay of a captured graph over overwritten frames; lengths=None = lengths all T; the
               single-clip methods = row 0 of the batch calls; a clip past 2^31 bytes of its buffer = that clip alone.
Small shapes: the planes are always 256 x 256, the sources a few dozen pixels."""
import numpy as np
import pytest
import torch

from tests import motion_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _video():
    from ultrafnd_git_amd import video
    return video


def _say(what, crit, err, bound):
    print(f"MOTION_ERR {what} {crit} err {float(err):.6e} bound {float(bound):.6e}")


def _run(frames, lengths=None, layout=None):
    """Both classes and the gray planes on one batch -> dict of host arrays."""
    v = _video()
    out = v.ChronosGuard(128).analyze_batch(frames, lengths, layout)
    out["flow256"], out["pooled"] = v.OpticalFlow3DCNN(256).extract_batch(frames, lengths, layout, return_pooled=True)
    out["flow512"] = v.OpticalFlow3DCNN(512).extract_batch(frames, lengths, layout)
    out["gray"] = v.ChronosGuard().gray_frames(frames, lengths, layout)
    return {k: t.cpu().numpy() for k, t in out.items()}


def _row(out, b, n):
    """Row b of a batch result, cut to a clip of n frames."""
    r = {k: a[b] for k, a in out.items()}
    r["gray"] = r["gray"][:n]
    for k in ("cut_scores", "flow_mags"):
        assert not r[k][max(n - 1, 0):].any(), k          # zero past the clip's last pair
        r[k] = r[k][:max(n - 1, 0)]
    return r


def _check(name, got, clip_u8, ref=None):
    """One clip's device results against the mirror (and, with `ref`, the reference's recorded numbers)."""
    g = R.gray(clip_u8)
    assert np.array_equal(got["gray"], g), name
    hist, pooled = R.hist32(g), R.pooled64(g)
    # exact
    assert np.array_equal(got["flow_mags"], R.flow_mags(g)), name
    cut32 = R.cut_scores64(hist).astype(np.float32) if len(g) > 1 else np.zeros(0, np.float32)
    d = R.ulp_distance32(got["cut_scores"], cut32)
    assert d.size == 0 or d.max() <= 1, (name, d)
    gp = got["pooled"].reshape(7, 11)
    assert np.array_equal(np.isnan(got["pooled"]), np.isnan(pooled["vector"])), name
    assert np.array_equal(gp[:, 3:], pooled["bins"].astype(np.float32)), name
    assert np.array_equal(gp[:, 2], pooled["max"].astype(np.float32), equal_nan=True), name
    # float statistics: float64 on the device's own series
    s64 = R.chronos_stats64(got["cut_scores"], got["flow_mags"])
    assert np.array_equal(np.isnan(got["stats"]), np.isnan(s64)), name
    fin = np.isfinite(s64)
    sb = R.chronos_bounds(got["cut_scores"], got["flow_mags"]) if len(g) > 1 else np.zeros(7)
    err = np.abs(got["stats"].astype(np.float64) - s64)
    for k, nm in enumerate(("cut_mean", "cut_std", "cut_max", "flow_mean", "flow_std", "flow_max", "corr")):
        if fin[k]:
            _say(f"chronos {name}", nm, err[k], sb[k])
            assert err[k] <= sb[k], (name, nm, err[k], sb[k])
    f64 = R.tile_normalise64(s64, 128)
    assert np.array_equal(np.isnan(got["features"]), np.isnan(f64)), name
    if fin.all():
        e, bnd = np.abs(got["features"] - f64).max(), R.vector_bound(s64, sb, 128)
        _say(f"chronos {name}", "features", e, bnd)
        assert e <= bnd, (name, e, bnd)
    t64 = R.tamper64(got["stats"].astype(np.float64)) if len(g) > 1 else 0.0
    _say(f"chronos {name}", "tamper", abs(float(got["tamper_score"]) - t64), R.U32)
    assert abs(float(got["tamper_score"]) - t64) <= R.U32, name            # a value in [0, 1] rounded to float32 once
    pb = R.pooled_bounds(pooled)
    pfin = np.isfinite(pooled["vector"])
    perr = np.abs(got["pooled"].astype(np.float64) - pooled["vector"])
    for c in range(7):
        for k, nm in ((0, "m_mean"), (1, "m_std")):
            if pfin[11 * c + k]:
                _say(f"flow {name} chunk{c}", nm, perr[11 * c + k], pb[11 * c + k])
                assert perr[11 * c + k] <= pb[11 * c + k], (name, c, nm, perr[11 * c + k], pb[11 * c + k])
    for key, dim in (("flow256", 256), ("flow512", 512)):
        v64 = R.tile_normalise64(pooled["vector"], dim) if len(g) > 1 else np.zeros(dim)
        assert np.array_equal(np.isnan(got[key]), np.isnan(v64)), (name, key)
        if pfin.all():
            e, bnd = np.abs(got[key] - v64).max(), R.vector_bound(pooled["vector"], pb, dim)
            _say(f"flow {name}", key, e, bnd)
            assert e <= bnd, (name, key, e, bnd)
    unequal = int((d != 0).sum())
    if ref is not None:      # the reference's recorded numbers
        assert np.array_equal(got["flow_mags"], ref["flows"]), name
        dr = R.ulp_distance32(got["cut_scores"], ref["cut_scores"])
        assert dr.max() <= 1, (name, dr)
        unequal = int((dr != 0).sum())
        want = ref["pooled"].reshape(7, 11)
        assert np.array_equal(gp[:, 2:], want[:, 2:], equal_nan=True), name
        for key in ("pooled", "flow256", "flow512", "features"):
            assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), (name, key)
    return unequal


def _same_bits(a, b, keys=("features", "tamper_score", "cut_scores", "flow_mags", "stats", "flow256", "flow512", "pooled", "gray")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return R.load_fixture(golden_dir / "motion.npz")


@pytest.fixture(scope="module")
def alone(fixture):
    """name -> the device's results for each fixture clip alone, HWC (computed once, shared, never modified)."""
    return {name: _row(_run(torch.from_numpy(ref["frames"]).to(DEV)[None]), 0, len(ref["frames"])) for name, ref in fixture.items()}


def test_fixture_parity_alone_hwc(fixture, alone):
    unequal = sum(_check(name, alone[name], ref["frames"], ref) for name, ref in fixture.items())
    print("cut scores not bit-equal to the reference's:", unequal)


def test_fixture_parity_chw_through_a_permuted_view(fixture, alone):
    for name, ref in fixture.items():
        hwc = torch.from_numpy(ref["frames"]).to(DEV)[None]
        view = hwc.permute(0, 1, 4, 2, 3)                                     # (1, T, 3, H, W): no copy
        assert view.data_ptr() == hwc.data_ptr() and _video().frame_layout(tuple(view.shape[2:])) == "CHW"
        _same_bits(_row(_run(view), 0, len(ref["frames"])), alone[name])
        packed = view.contiguous()                                             # and a genuinely planar tensor
        _same_bits(_row(_run(packed), 0, len(ref["frames"])), alone[name])


def test_fixture_parity_in_one_ragged_batch(fixture, alone):
    """All fixture clips in one batch through `lengths`.  One tensor holds one source size, so each clip enters as its own
    nearest-neighbour 256 x 256 RGB resize -- at that size the resize is the identity, hence the same gray planes as its source."""
    names = list(fixture)
    T = max(len(fixture[n]["frames"]) for n in names)
    batch = torch.zeros(len(names), T, 256, 256, 3, dtype=torch.uint8)
    for b, n in enumerate(names):
        f = fixture[n]["frames"]
        iy, ix = R.source_index(f.shape[1]), R.source_index(f.shape[2])
        batch[b, :len(f)] = torch.from_numpy(f[:, iy][:, :, ix])
        batch[b, len(f):] = 255 - batch[b, :1]                                 # junk past the end: must not be read
    lens = torch.tensor([len(fixture[n]["frames"]) for n in names], dtype=torch.int32, device=DEV)
    out = _run(batch.to(DEV), lens)
    for b, n in enumerate(names):
        row = _row(out, b, len(fixture[n]["frames"]))
        _same_bits(row, alone[n])
        _check(n, row, fixture[n]["frames"], fixture[n])


def test_luma_on_all_2_24_triples():
    """One clip of 256 frames of 256 x 256 (the resize is the identity) whose pixels enumerate every (r, g, b)."""
    r, g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    clip = np.stack([r, g, b], axis=-1)                                        # frame = r, row = g, column = b
    got = _video().ChronosGuard().gray_frames(torch.from_numpy(clip).to(DEV)[None])[0].cpu().numpy()
    want = R.luma(clip)
    bad = int((got != want).sum())
    print("luma: triples that differ from the float64 expression:", bad)
    assert bad == 0
    integer = ((2989 * r.astype(np.int64) + 5870 * g.astype(np.int64) + 1140 * b.astype(np.int64)) // 10000).astype(np.uint8)
    assert (integer != want).sum() == 296                                      # the triples an integer formula gets wrong


@pytest.mark.parametrize("H,W", [(1, 1), (255, 257), (256, 256), (257, 255), (40, 48), (300, 500)])
def test_resize_edges(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    clip = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    dev = torch.from_numpy(clip).to(DEV)[None]
    v = _video()
    want = R.gray(clip)
    assert np.array_equal(v.ChronosGuard().gray_frames(dev)[0].cpu().numpy(), want)
    assert np.array_equal(v.ChronosGuard().gray_frames(dev.permute(0, 1, 4, 2, 3))[0].cpu().numpy(), want)
    sliced = torch.from_numpy(rng.integers(0, 256, (1, 3, H + 3, W + 5, 3), dtype=np.uint8)).to(DEV)      # a strided window of a larger frame
    win = sliced[:, :, 2:2 + H, 4:4 + W]
    assert np.array_equal(v.ChronosGuard().gray_frames(win)[0].cpu().numpy(), R.gray(win[0].cpu().numpy()))


TIMES = (1, 2, 4, 5, 6, 9, 12)


def _time_clip(T):
    rng = np.random.default_rng(100 + T)
    base = rng.integers(0, 256, (9, 11, 3)).astype(np.float64)
    return np.stack([np.clip(base * gain + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8) for gain in rng.uniform(0.3, 1.0, T)])


def test_time_edges_alone_and_ragged():
    """T = 1, 2, 4, 5, 6, 9, 12: 0, 1, 3, 4, 5, 8, 11 pairs -- around the pyramid's boundaries at 4, 8 and 11 pairs."""
    clips = {T: _time_clip(T) for T in TIMES}
    single = {}
    for T, clip in clips.items():
        single[T] = _row(_run(torch.from_numpy(clip).to(DEV)[None]), 0, T)
        _check(f"T{T}", single[T], clip)
    assert not single[1]["features"].any() and not single[1]["flow256"].any() and single[1]["tamper_score"] == 0       # fewer than 2 frames
    assert np.isnan(single[2]["flow256"]).all() and np.isnan(single[4]["flow256"]).all() and np.isfinite(single[5]["flow256"]).all()
    assert np.isfinite(single[4]["features"]).all()
    batch = torch.zeros(len(TIMES), max(TIMES), 9, 11, 3, dtype=torch.uint8)
    for b, T in enumerate(TIMES):
        batch[b, :T] = torch.from_numpy(clips[T])
        batch[b, T:] = 200
    out = _run(batch.to(DEV), torch.tensor(TIMES, dtype=torch.int32, device=DEV))
    for b, T in enumerate(TIMES):
        _same_bits(_row(out, b, T), single[T])


def test_static_clip_gives_the_references_nan(fixture, alone):
    a = alone["static6"]
    assert np.isnan(a["features"]).all() and np.isnan(a["stats"][6]) and np.isfinite(a["stats"][:6]).all() and a["tamper_score"] == 0.0
    assert np.isfinite(a["flow256"]).all() and not a["cut_scores"].any() and not a["flow_mags"].any()
    assert float(a["tamper_score"]) == float(fixture["static6"]["tamper"])


def test_bit_comparisons(fixture, alone):
    v = _video()
    names = ("rand7", "cut9", "long12")
    clips = {n: torch.from_numpy(fixture[n]["frames"]).to(DEV) for n in names}
    a = clips["rand7"]
    # rerun
    _same_bits(_row(_run(a[None]), 0, 7), alone["rand7"])
    # inside a batch of 3 of the same source size, any position
    b3 = torch.stack([torch.flip(a, dims=(0,)), a, torch.roll(a, 2, 0)])
    _same_bits(_row(_run(b3), 1, 7), alone["rand7"])
    # lengths=None equals lengths all T
    full = _run(b3, torch.full((3,), 7, dtype=torch.int32, device=DEV))
    _same_bits(full, _run(b3))
    # one call for both classes: the same bits
    both = {k: t.cpu().numpy() for k, t in v.motion_features(a[None], feat_dim=128, dim=256).items()}
    for k, k2 in (("features", "features"), ("tamper_score", "tamper_score"), ("cut_scores", "cut_scores"), ("flow_mags", "flow_mags"), ("flow", "flow256"),
                  ("pooled", "pooled")):
        assert np.array_equal(both[k][0][:6] if k in ("cut_scores", "flow_mags") else both[k][0], alone["rand7"][k2], equal_nan=True), k
    # the single-clip methods: row 0 of the batch calls; host arrays are taken as the reference takes them
    guard, flow = v.ChronosGuard(128), v.OpticalFlow3DCNN(256)
    assert np.array_equal(guard.extract_features(a), alone["rand7"]["features"]) and np.array_equal(flow.extract(a), alone["rand7"]["flow256"])
    assert guard.temporal_tamper_score(a) == float(alone["rand7"]["tamper_score"])
    assert np.array_equal(flow.extract(fixture["rand7"]["frames"]), alone["rand7"]["flow256"])
    assert np.array_equal(guard.extract_features(list(fixture["rand7"]["frames"])), alone["rand7"]["features"])
    # a captured graph replayed after the frames were overwritten in place
    static = torch.from_numpy(fixture["cut9"]["frames"]).to(DEV)[None].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        v.motion_features(static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = v.motion_features(static)
    rng = np.random.default_rng(8)
    other = np.clip(fixture["cut9"]["frames"].astype(np.int32) + rng.integers(-40, 41, fixture["cut9"]["frames"].shape), 0, 255).astype(np.uint8)
    for frames_np in (other, fixture["cut9"]["frames"]):
        static.copy_(torch.from_numpy(frames_np).to(DEV)[None])
        graph.replay()
        torch.cuda.synchronize()
        eager = _row(_run(torch.from_numpy(frames_np).to(DEV)[None]), 0, 9)
        for k, k2 in (("features", "features"), ("tamper_score", "tamper_score"), ("cut_scores", "cut_scores"), ("flow_mags", "flow_mags"),
                      ("flow", "flow256"), ("pooled", "pooled"), ("stats", "stats")):
            assert np.array_equal(out[k][0].cpu().numpy(), eager[k2], equal_nan=True), k
    _same_bits(eager, alone["cut9"])


def test_float_frames_follow_the_per_frame_rule():
    """A clip mixing frames in [0, 1] with frames in 0..255 (and values outside): equal to the uint8 clip the mirror's conversion gives."""
    rng = np.random.default_rng(4)
    f = np.stack([rng.random((10, 12, 3)), rng.random((10, 12, 3)) * 300 - 20, rng.random((10, 12, 3)), np.full((10, 12, 3), 1.0),
                  rng.random((10, 12, 3)) * 255, rng.random((10, 12, 3)) * 0.5]).astype(np.float32)
    u8 = R.to_uint8(f)
    v = _video()
    dev = torch.from_numpy(f).to(DEV)[None]
    assert np.array_equal(v.frames_to_uint8(dev)[0].cpu().numpy(), u8)
    _same_bits(_run(dev), _run(torch.from_numpy(u8).to(DEV)[None]))
    chw = dev.permute(0, 1, 4, 2, 3).contiguous()
    _same_bits(_run(chw), _run(torch.from_numpy(u8).to(DEV)[None]))


def test_offsets_past_2_31_bytes():
    """Two small clips in one flat buffer, the second starting past 2^31 bytes: row 1 equals that clip alone."""
    T, H, W = 6, 10, 12
    clip_bytes = T * H * W * 3
    gap = (1 << 31) + 64
    flat = torch.empty(gap + clip_bytes, dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(6)
    c0, c1 = (torch.from_numpy(rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)).to(DEV) for _ in range(2))
    flat[:clip_bytes] = c0.reshape(-1)
    flat[gap:] = c1.reshape(-1)
    view = torch.as_strided(flat, (2, T, H, W, 3), (gap, H * W * 3, W * 3, 3, 1))
    out = _run(view)
    _same_bits(_row(out, 0, T), _row(_run(c0[None]), 0, T))
    _same_bits(_row(out, 1, T), _row(_run(c1[None]), 0, T))
    _check("past2^31", _row(out, 1, T), c1.cpu().numpy())


def test_cache_visual(fixture):
    v = _video()
    for name in ("rand7", "down5", "four4"):
        ref = fixture[name]
        got = v.cache_visual(torch.from_numpy(ref["frames"]).to(DEV)[None])[0].cpu().numpy()
        want32 = ref["flow512"] / (np.linalg.norm(ref["flow512"]) + 1e-9)      # the cache's l2n of the reference's own dim = 512 vector
        assert np.array_equal(np.isnan(got), np.isnan(want32)), name
        if name == "four4":
            continue
        pooled = R.pooled64(R.gray(ref["frames"]))
        v64 = R.tile_normalise64(pooled["vector"], 512)
        v64 = v64 / (np.linalg.norm(v64) + 1e-9)
        # the flow vector's bound vb per entry, then a second normalisation: the norm of a vector whose entries are off by vb moves by
        # at most sqrt(dim) vb, its float32 evaluation by (dim / 2 + 3) u, both relative to an entry <= amax.  Against the reference's
        # own float32 row, which obeys the same bound: twice that.
        vb, amax = R.vector_bound(pooled["vector"], R.pooled_bounds(pooled), 512), np.abs(v64).max()
        bound = 1.01 * (vb + amax * (np.sqrt(512) * vb + (512 / 2 + 3) * R.U32))
        for what, other, k in (("float64", v64, 1), ("reference", want32.astype(np.float64), 2)):
            e = np.abs(got - other).max()
            _say(f"cache_visual {name}", what, e, k * bound)
            assert e <= k * bound, (name, what, e, k * bound)
