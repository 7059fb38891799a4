"""GPU: batched A/V lag estimation (csrc/av_lag.hip, ultrafnd_git_amd/temporal.py: av_lag) against the REFERENCE's own answers
(tests/golden/avlag.npz, minted from its two estimate_av_lag functions), against the exact fp32 mirror of the documented summation
order (tests/avlag_ref.py; every standardised sample and every finite correlation value up to n = 4099), against the float64
restatement at the derived radii, and bit for bit against itself: alone = ragged batch with NaN behind every row's length = rerun =
replayed hipGraph = any `want` subset = both classes' estimate_av_lag_batch; a strided row view = its contiguous copy.

Beside the fixture's cases: n either side of one 2048-sample segment, and windows of 511 / 513 and 1023 / 1025 lags (either side of a
wave's 512 lags and of a workgroup's 1024).  The restatement, the radii, the mirror and every device result are computed once per
module and shared, unchanged, by the tests.  Nothing here reads the reference tree.

Measured on an MI355X (profiles/avlag_errors.txt): no value differs from the mirror; the worst |value - float64| over its radius is
0.94 for a_std, 0.80 for m_std, 0.37 for xcorr, 0.19 for peak_corr."""
from pathlib import Path

import numpy as np
import pytest
import torch

import avlag_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("lag_samples", "lag_seconds", "peak_corr", "xcorr", "a_std", "m_std")
FIXTURE = Path(__file__).resolve().parent / "golden" / "avlag.npz"
MIRROR_MAX = 4099


def _cpu(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _padded(rows, fill=float("nan")):
    """(B, n_max) host batch: every row followed by `fill` (NaN: whatever is read at or past a row's length poisons its results)."""
    batch = torch.full((len(rows), max(max(len(r) for r in rows), 1)), fill, dtype=torch.float32)
    for i, r in enumerate(rows):
        batch[i, :len(r)] = torch.from_numpy(r)
    return batch


def _entries():
    """name -> {"a", "m", "sr", "max_lag_s", "kind", "seconds" (fixture entries only)}."""
    out = {}
    for name, c in R.load_fixture(FIXTURE).items():
        out[name] = dict(c)
    out["n125_k0"] = {**out["n125_sr100"], "sr": 16000.0, "max_lag_s": 0.0, "seconds": None}
    rng = np.random.default_rng(77)

    def pair(n, shift):
        base = np.convolve(rng.standard_normal(n + 2 * abs(shift) + 2), [0.25, 0.5, 0.25], "valid")
        p = abs(shift)
        m = (0.6 + 0.25 * base[p:p + n]).astype(np.float32)
        a = (1.0 + 0.2 * base[p - shift:p - shift + n] + 0.02 * rng.standard_normal(n)).astype(np.float32)
        return a, m

    for n, shift in ((2047, 17), (2048, -33), (2049, 40)):      # either side of one segment; sr = 1: K = int(max_lag_s)
        a, m = pair(n, shift)
        out[f"seg_n{n}"] = {"a": a, "m": m, "sr": 1.0, "max_lag_s": 40.0, "kind": "regular", "seconds": None, "fps": 25.0}
    for K in (255, 256, 511, 512):      # 2 K + 1 lags: either side of a wave's 512 and of a workgroup's 1024
        for n, shift in ((600, K - 3), (777, -(K // 2))):
            a, m = pair(n, shift)
            out[f"lags_k{K}_n{n}"] = {"a": a, "m": m, "sr": 1.0, "max_lag_s": float(K), "kind": "regular", "seconds": None, "fps": 25.0}
    return out


@pytest.fixture(scope="module")
def world():
    from ultrafnd_git_amd import temporal
    ent = _entries()
    alone, w64, rad, mir = {}, {}, {}, {}
    for name, e in ent.items():
        K = R.max_lag(e["sr"], e["max_lag_s"])
        a, m = torch.from_numpy(e["a"])[None].to(DEV), torch.from_numpy(e["m"])[None].to(DEV)
        alone[name] = _cpu(temporal.av_lag(a, m, None, None, e["sr"], 25.0, e["max_lag_s"], ALL))
        w64[name] = R.window64(e["a"], e["m"], K)
        rad[name] = R.radii(e["a"], e["m"], K) if e["kind"] in ("regular", "outside") else None
        mir[name] = R.mirror(e["a"], e["m"], K) if min(e["a"].size, e["m"].size) <= MIRROR_MAX else None
    groups = {}
    for name, e in ent.items():
        groups.setdefault((e["sr"], e["max_lag_s"]), []).append(name)
    batches = []
    for (sr, max_lag_s), names in groups.items():
        names = names[::2] + names[1::2]      # neighbours in a batch differ in length
        for at in range(0, len(names), 6):
            group = names[at:at + 6]
            if len(group) < 2:
                group = group + names[:1]
            if not batches:
                group = group[:1] + [None] + group[1:]      # a pair of length 0 inside the first batch
            rows_a = [ent[n]["a"] if n else np.zeros(0, np.float32) for n in group]
            rows_m = [ent[n]["m"] if n else np.zeros(0, np.float32) for n in group]
            A, M = _padded(rows_a).to(DEV), _padded(rows_m).to(DEV)
            la = torch.tensor([len(r) for r in rows_a], dtype=torch.int32, device=DEV)
            lm = torch.tensor([len(r) for r in rows_m], dtype=torch.int32, device=DEV)
            batches.append({"group": group, "A": A, "M": M, "la": la, "lm": lm, "sr": sr, "max_lag_s": max_lag_s,
                            "out": _cpu(temporal.av_lag(A, M, la, lm, sr, 25.0, max_lag_s, ALL))})
    return {"ent": ent, "alone": alone, "w64": w64, "rad": rad, "mir": mir, "batches": batches}


def _views(world):
    """(name, where, outputs of one pair) for every pair alone and for every row of every ragged batch."""
    for name, o in world["alone"].items():
        yield name, "alone", {k: v[0] for k, v in o.items()}
    for b in world["batches"]:
        for r, name in enumerate(b["group"]):
            if name:
                yield name, "batch", {k: v[r] for k, v in b["out"].items()}


def _geometry(world, name):
    e = world["ent"][name]
    K = R.max_lag(e["sr"], e["max_lag_s"])
    n = min(e["a"].size, e["m"].size)
    return e, K, n, min(K, n - 1)


def _cut(world, name, o):
    """The pair's own part of every output: a_std / m_std up to n (zeros from there on, asserted), xcorr's window (-inf outside it,
    asserted; finite inside)."""
    e, K, n, Kc = _geometry(world, name)
    out = dict(o)
    for k in ("a_std", "m_std"):
        assert not o[k][n:].any(), (name, k)
        out[k] = o[k][:n]
    x = o["xcorr"]
    assert x.shape == (2 * K + 1,)
    inside = np.abs(np.arange(2 * K + 1) - K) <= Kc if n >= 4 else np.zeros(2 * K + 1, bool)
    assert np.isneginf(x[~inside]).all() and np.isfinite(x[inside]).all(), name
    out["xcorr"] = x[inside]
    return out


def test_every_batch_is_ragged_and_every_case_and_edge_is_there(world):
    assert all(len(b["group"]) >= 2 for b in world["batches"])
    assert any(len(set(b["la"].tolist())) > 1 for b in world["batches"]) and None in world["batches"][0]["group"]
    assert {n for b in world["batches"] for n in b["group"] if n} == set(world["ent"])
    n = {_geometry(world, name)[2] for name in world["ent"]}
    assert {3, 4, 5, 16, 63, 64, 65, 125, 257, 1000, 4099, 20000, R.SEG - 1, R.SEG, R.SEG + 1} <= n
    lags = {2 * _geometry(world, name)[1] + 1 for name in world["ent"]}
    assert {R.WAVE_LAGS - 1, R.WAVE_LAGS + 1, R.LAG_BLOCK - 1, R.LAG_BLOCK + 1, 1} <= lags
    assert world["alone"]["la300_lm257"]["a_std"].shape == (1, 257) and world["alone"]["la125_lm200"]["m_std"].shape == (1, 125)      # na_max != nm_max


def test_lag_equals_the_reference_s_fixture_exactly(world):
    seen = set()
    for name, where, o in _views(world):
        e = world["ent"][name]
        if e["seconds"] is None:
            continue
        seen.add((name, where))
        assert o["lag_seconds"].dtype == np.float64 and o["lag_samples"].dtype == np.int32
        assert float(o["lag_seconds"]) == e["seconds"], (name, where, float(o["lag_seconds"]), e["seconds"])
        assert int(o["lag_samples"]) == round(e["seconds"] * e["sr"]) and float(o["lag_seconds"]) == int(o["lag_samples"]) / e["sr"], (name, where)
    assert len({n for n, _ in seen}) >= 21 and {w for _, w in seen} == {"alone", "batch"}


def test_standardised_rows_and_correlations_equal_the_fp32_mirror_bit_for_bit(world):
    """Every standardised sample, every finite xcorr value, the lag and the peak: the documented order, none excluded."""
    checked = 0
    for name, where, o in _views(world):
        mir = world["mir"][name]
        e, K, n, Kc = _geometry(world, name)
        if n < 4 or n > MIRROR_MAX:
            assert mir is None
            continue
        o = _cut(world, name, o)
        for k, want in (("a_std", mir["a_std"]), ("m_std", mir["m_std"]), ("xcorr", mir["c"])):
            same = o[k].view(np.uint32) == want.view(np.uint32)
            assert same.all(), (name, where, k, int((~same).sum()), same.size)
        assert int(o["lag_samples"]) == mir["lag"] and o["peak_corr"].view(np.uint32) == mir["peak"].view(np.uint32), (name, where)
        checked += 1
    assert checked >= 2 * 30


def test_every_value_lies_within_its_radius_of_float64_and_the_lag_is_a_possible_one(world):
    worst = {k: 0.0 for k in ("a_std", "m_std", "xcorr", "peak_corr")}
    for name, where, o in _views(world):
        w, rad = world["w64"][name], world["rad"][name]
        if rad is None:
            continue
        e, K, n, Kc = _geometry(world, name)
        o = _cut(world, name, o)
        for k, c, r in (("a_std", w["a_std"], rad["a_std"]), ("m_std", w["m_std"], rad["m_std"]), ("xcorr", w["c"], rad["c"])):
            err = np.abs(o[k].astype(np.float64) - c)
            assert (err <= r).all(), (name, where, k, float((err / r).max()))      # no entry is excluded
            worst[k] = max(worst[k], float((err / r).max()))
        lag = int(o["lag_samples"])
        assert lag in R.possible_lags(w["c"], rad["c"], Kc).tolist(), (name, where, lag)
        j = lag + Kc
        err = abs(float(o["peak_corr"]) - w["c"][j] / n)
        assert err <= rad["peak"][j], (name, where, err, rad["peak"][j])
        assert o["peak_corr"] == np.float32(o["xcorr"][j] / np.float32(n)) and o["xcorr"][j] == o["xcorr"].max(), (name, where)
        assert -1.0 - 1e-3 <= float(o["peak_corr"]) <= 1.0 + 1e-3
        worst["peak_corr"] = max(worst["peak_corr"], err / rad["peak"][j])
    print("worst |value - float64| / radius:", worst)


def test_constant_rows_give_exact_zeros_and_the_first_lag_of_the_window(world):
    seen = 0
    for name, where, o in _views(world):
        if world["ent"][name]["kind"] not in ("zero_a", "const_half"):
            continue
        e, K, n, Kc = _geometry(world, name)
        o = _cut(world, name, o)
        assert not o["a_std"].view(np.uint32).any() and not o["xcorr"].view(np.uint32).any(), (name, where)      # +0, every bit
        assert int(o["lag_samples"]) == -Kc and float(o["lag_seconds"]) == -Kc / e["sr"] and o["peak_corr"].view(np.uint32) == 0, (name, where)
        assert o["m_std"].any()
        seen += 1
    assert seen == 6


def test_fewer_than_four_samples_give_zero_and_rows_of_minus_infinity(world):
    rows = [(name, where, o) for name, where, o in _views(world) if name == "n3"]
    b = world["batches"][0]
    rows.append(("empty", "batch", {k: v[b["group"].index(None)] for k, v in b["out"].items()}))
    assert len(rows) == 3
    for name, where, o in rows:
        assert int(o["lag_samples"]) == 0 and float(o["lag_seconds"]) == 0.0 and o["peak_corr"].view(np.uint32) == 0, (name, where)
        assert np.isneginf(o["xcorr"]).all() and o["xcorr"].size == 16001 and not o["a_std"].any() and not o["m_std"].any(), (name, where)


def test_a_pair_alone_equals_its_row_of_a_ragged_batch_bit_for_bit(world):
    """The batch rows carry NaN behind every row's length: nothing at or past it reaches a result."""
    for b in world["batches"]:
        for r, name in enumerate(b["group"]):
            if not name:
                continue
            a = _cut(world, name, {k: v[0] for k, v in world["alone"][name].items()})
            row = _cut(world, name, {k: v[r] for k, v in b["out"].items()})
            for k in ALL:
                assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], row[k].view(np.uint32) if row[k].dtype == np.float32 else row[k]), (name, k)


def _batch(world, name):
    return next(b for b in world["batches"] if name in b["group"])


def test_rerun_graph_replay_output_subsets_and_both_classes_give_the_same_bits(world):
    from ultrafnd_git_amd import temporal
    from ultrafnd_git_amd.video import ChronosGuard
    b = _batch(world, "n4099")
    args = (b["la"], b["lm"], b["sr"], 25.0, b["max_lag_s"])
    first = temporal.av_lag(b["A"], b["M"], *args, ALL)
    for k in ALL:
        assert np.array_equal(first[k].cpu().numpy(), b["out"][k], equal_nan=True), k      # = the module's run
    eq = lambda x, y: torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    for want in (("lag_seconds",), ("lag_samples",), ("peak_corr",), ("xcorr",), ("a_std",), ("m_std", "a_std"), ("xcorr", "lag_samples"),
                 ("peak_corr", "lag_seconds", "m_std")):
        sub = temporal.av_lag(b["A"], b["M"], *args, want)
        assert tuple(sub) == tuple(k for k in ALL if k in want)      # what was not asked for is not stored
        for k in want:
            assert eq(sub[k], first[k]), (want, k)
    for fn in (temporal.TemporalSyncNet.estimate_av_lag_batch, ChronosGuard.estimate_av_lag_batch):
        got = fn(b["A"], b["M"], *args, ALL)
        for k in ALL:
            assert eq(got[k], first[k]), (fn.__qualname__, k)
    assert tuple(temporal.av_lag(b["A"], b["M"], b["la"], b["lm"])) == ("lag_seconds",)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()      # a captured call, replayed on new content of the same buffers
    As, Ms, las, lms = b["A"].clone(), b["M"].clone(), b["la"].clone(), b["lm"].clone()
    with torch.cuda.graph(graph):
        held = temporal.av_lag(As, Ms, las, lms, b["sr"], 25.0, b["max_lag_s"], ALL)
    perm = list(range(1, len(b["group"]))) + [0]
    for dst, src in ((As, b["A"]), (Ms, b["M"]), (las, b["la"]), (lms, b["lm"])):
        dst.copy_(src[perm])
    graph.replay()
    torch.cuda.synchronize()
    for k in ALL:
        assert eq(held[k], first[k][perm]), k


def test_a_strided_row_view_equals_its_contiguous_copy_and_sequences_equal_tensors(world):
    from ultrafnd_git_amd import temporal
    b = _batch(world, "n1000_plus")
    B, na = b["A"].shape
    wide_a = torch.full((B, na + 37), float("nan"), device=DEV)
    wide_m = torch.full((B, 2 * b["M"].shape[1]), float("nan"), device=DEV)
    wide_a[:, :na] = b["A"]
    wide_m[:, :b["M"].shape[1]] = b["M"]
    va, vm = wide_a[:, :na], wide_m[:, :b["M"].shape[1]]
    assert not va.is_contiguous() and va.stride(0) == na + 37 and va.data_ptr() == wide_a.data_ptr()
    got = temporal.av_lag(va, vm, b["la"], b["lm"], b["sr"], 25.0, b["max_lag_s"], ALL)
    lists = temporal.av_lag(b["A"], b["M"], b["la"].tolist(), b["lm"].tolist(), b["sr"], 25.0, b["max_lag_s"], ALL)
    for k in ALL:
        assert np.array_equal(got[k].cpu().numpy(), b["out"][k], equal_nan=True), k
        assert np.array_equal(lists[k].cpu().numpy(), b["out"][k], equal_nan=True), k
    # lengths beyond the row width and below zero are clamped on the device
    r = b["group"].index("n1000_plus")
    ra, rm = b["A"][r:r + 1, :500], b["M"][r:r + 1, :400]
    full = temporal.av_lag(ra, rm, [10 ** 6], [10 ** 6], b["sr"], 25.0, b["max_lag_s"], ALL)
    none = temporal.av_lag(ra, rm, None, None, b["sr"], 25.0, b["max_lag_s"], ALL)
    neg = temporal.av_lag(ra, rm, [-5], None, b["sr"], 25.0, b["max_lag_s"], ("lag_samples", "xcorr"))
    assert torch.isfinite(none["a_std"]).all() and none["a_std"].shape == (1, 400)
    for k in ALL:
        assert np.array_equal(full[k].cpu().numpy(), none[k].cpu().numpy(), equal_nan=True), k
    assert int(neg["lag_samples"][0]) == 0 and torch.isneginf(neg["xcorr"]).all()
