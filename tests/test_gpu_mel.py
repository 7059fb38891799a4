"""GPU: the librosa-branch mel spectrogram in dB (csrc/mel_db.hip, ultrafnd_git_amd/audio.py): its mel powers against the exact fp32
mirror of the filterbank chain applied to the magnitudes spectral_descriptors returns (every value), its dB against the float64
formula on its own powers, everything against the float64 restatement at the interval bounds of tests/mel_ref.py, the clip-wide
maximum across tile boundaries, and bit for bit against itself: alone = ragged batch with NaN behind every clip = rerun = replayed
hipGraph = any set of outputs = the class, row for row.

Nothing is compared with librosa (it is not part of this environment) and there is no fixture of the reference for this branch.
The restatement, its bounds, the mirror and every device result are computed once per module and shared, unchanged, by the tests.

Measured on an MI355X (profiles/mel_errors.txt): no mel power differs from the mirror; the worst |value - float64| over the radius
of its bound is 0.0099 for mel_db, 0.011 for mel_power, 0.0088 for mel_max."""
import numpy as np
import pytest
import torch

import mel_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = ("mel_db", "mel_power", "mel_max")
# lengths where the tiling can go wrong: a single sample, either side of a hop, one frame either side of one 64-frame tile
# (T = 64 | 65) and of two (T = 128 | 129: two full tiles and one frame)
EDGE_LENGTHS = (1, 159, 160, 161, 64 * 160 - 1, 64 * 160, 128 * 160 - 1, 128 * 160)
ULP_100 = 2.0 ** -17      # one fp32 ulp at |D| in [64, 128)


def _cpu(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _padded(waves, fill=float("nan")):
    """(B, n_max) host batch: every clip followed by `fill` (NaN: whatever is read past a clip's length poisons its results)."""
    batch = torch.full((len(waves), max(max(len(w) for w in waves), 1)), fill, dtype=torch.float32)
    for r, w in enumerate(waves):
        batch[r, :len(w)] = torch.from_numpy(w)
    return batch


@pytest.fixture(scope="module")
def world():
    """clips (the restatement's five cases plus seeded noise at the edge lengths), their bounds, the device results of every clip
    alone (with the magnitudes of spectral_descriptors and the mirror on them) and of ragged batches of 3 to 6 clips, one of which
    also holds a clip of length 0."""
    from ultrafnd_git_amd import audio
    rng = np.random.default_rng(164)
    clips = dict(M.cases())
    for n in EDGE_LENGTHS:
        clips[f"len{n}"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
    fb = audio.mel_filterbank()
    bounds, alone, mags, mirror = {}, {}, {}, {}
    for name, x in clips.items():
        xd = torch.from_numpy(x)[None].to(DEV)
        bounds[name] = M.bounds(x)
        alone[name] = _cpu(audio.mel_spectrogram(xd, None, ALL))
        mags[name] = audio.spectral_descriptors(xd, None, want=("magnitude",))["magnitude"].cpu().numpy()[0]
        mirror[name] = M.mel_power_mirror(mags[name], fb["weights"], fb["first"], fb["count"])
    names = list(clips)
    order = names[::2] + names[1::2]      # neighbours in a batch differ in kind and length
    sizes, batches, at = (5, 3, 4, 6), [], 0
    while at < len(order):
        group = order[at:at + sizes[len(batches) % len(sizes)]]
        at += len(group)
        if len(group) < 3:      # (the tail joins clips already seen: every batch holds 3 to 6)
            group = group + order[:3 - len(group)]
        if not batches:
            group = group[:2] + [None] + group[2:]      # a clip of length 0 inside the first batch
        waves = [clips[n] if n else np.zeros(0, np.float32) for n in group]
        x = _padded(waves).to(DEV)
        lens = torch.tensor([len(w) for w in waves], dtype=torch.int32, device=DEV)
        batches.append((group, x, lens, _cpu(audio.mel_spectrogram(x, lens, ALL))))
    return {"clips": clips, "bounds": bounds, "alone": alone, "mags": mags, "mirror": mirror, "batches": batches}


def _views(world):
    """(name, where, outputs of one clip) for every clip alone and for every row of every ragged batch."""
    for name, o in world["alone"].items():
        yield name, "alone", {k: v[0] for k, v in o.items()}
    for group, _, _, o in world["batches"]:
        for r, name in enumerate(group):
            if name:
                yield name, "batch", {k: v[r] for k, v in o.items()}


def _cut(world, name, o):
    """The clip's own frames of the per-frame outputs; asserts zeros from there on."""
    T = M.frame_counts(len(world["clips"][name]))[0]
    out = dict(o)
    for k in ("mel_db", "mel_power"):
        assert not o[k][:, T:].any(), (name, k)
        out[k] = o[k][:, :T]
    return out


def test_every_batch_is_ragged_and_every_edge_length_is_there(world):
    assert all(3 <= len(g) <= 6 and len(set(lens.tolist())) > 1 for g, _, lens, _ in world["batches"])
    seen = {n for g, _, _, _ in world["batches"] for n in g if n}
    assert seen == set(world["clips"]) and None in world["batches"][0][0]
    T = {M.frame_counts(len(x))[0] for x in world["clips"].values()}
    assert {1, 2, 64, 65, 128, 129, 130} <= T


def test_mel_power_is_the_exact_chain_on_the_magnitudes_of_spectral_descriptors(world):
    """One value, one arithmetic: the magnitudes under the mel are the bits spectral_descriptors returns, and every mel power is the
    fmaf chain over its filter's support on them.  Every value, none excluded."""
    for name, where, o in _views(world):
        o = _cut(world, name, o)
        T = o["mel_power"].shape[1]
        want = world["mirror"][name][:, :T]
        assert world["mags"][name].shape[1] == T or not world["mags"][name][:, T:].any()
        same = o["mel_power"].view(np.uint32) == want.view(np.uint32)
        assert same.all(), (name, where, int((~same).sum()), same.size)


def test_db_is_the_float64_formula_on_the_device_s_own_powers(world):
    """mel_db is within one fp32 ulp of the float64 formula on the device's mel_power and mel_max (plus 2^-44: two double log10 of
    magnitude <= 100, each within an ulp of 2^-46 of the other routine's, and their difference); exactly -80 wherever the float64
    value is below -80 - 2^-17; mel_max is the maximum of the clip's own powers, exactly."""
    for name, where, o in _views(world):
        o = _cut(world, name, o)
        assert o["mel_max"] == o["mel_power"].max(), (name, where)
        ref = M.db_of_device(o["mel_power"], o["mel_max"])
        raw = 10.0 * np.log10(np.maximum(1e-10, o["mel_power"].astype(np.float64))) - 10.0 * np.log10(max(1e-10, float(o["mel_max"])))
        err = np.abs(o["mel_db"].astype(np.float64) - ref)
        tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 2.0 ** -44
        assert (tol <= ULP_100 + 2.0 ** -44).all() and (err <= tol).all(), (name, where, float((err / tol).max()))
        assert (o["mel_db"][raw < -80.0 - ULP_100] == np.float32(-80.0)).all(), (name, where)
        assert o["mel_db"].max() == 0.0 and o["mel_db"].min() >= -80.0, (name, where)


def test_every_value_lies_inside_its_interval_bound(world):
    worst = {k: 0.0 for k in ALL}
    for name, where, o in _views(world):
        o, b = _cut(world, name, o), world["bounds"][name]
        for k in ALL:
            v = np.asarray(o[k], dtype=np.float64)
            assert np.isfinite(v).all(), (name, where, k)
            ok = M.inside(v, b[k])      # no entry is excluded
            assert ok.all(), (name, where, k, v[~ok][:4], np.asarray(b[k][0])[~ok][:4], np.asarray(b[k][1])[~ok][:4])
            c = np.asarray(b["center"][k], dtype=np.float64)
            rad = np.maximum(np.asarray(b[k][1]) - c, c - np.asarray(b[k][0]))
            worst[k] = max(worst[k], float(np.max(np.where(rad > 0, np.abs(v - c) / np.where(rad > 0, rad, 1.0), 0.0))))
    print("worst |value - float64| / radius of its bound:", worst)


def test_the_reference_maximum_is_the_clip_s_not_the_tile_s(world):
    """quiet_then_loud: the first tile is 54 dB below the last.  With a per-tile reference frame 0 would peak at 0 dB."""
    for name, where, o in _views(world):
        if name == "quiet_then_loud":
            D = o["mel_db"]
            assert D[:, 128:130].max() == 0.0 and D[:, 0].max() <= -40.0 and D[:, :64].max() <= -40.0, where
    assert {w for n, w, _ in _views(world) if n == "quiet_then_loud"} == {"alone", "batch"}


def test_all_zero_clips_padding_and_the_clip_of_length_zero(world):
    for name, where, o in _views(world):
        o = _cut(world, name, o)      # (asserts the zeros from T on)
        if name == "zeros":
            assert not o["mel_db"].any() and not o["mel_power"].any() and o["mel_max"] == 0.0 and o["mel_db"].shape == (64, 26), where
    group, _, _, out = world["batches"][0]
    r = group.index(None)
    for k in ALL:
        assert not out[k][r].any(), k


def test_a_clip_alone_equals_its_row_of_a_ragged_batch_bit_for_bit(world):
    """The batch rows carry NaN behind every clip: nothing at or past x[len] reaches a result."""
    for group, _, _, out in world["batches"]:
        for r, name in enumerate(group):
            if not name:
                continue
            a = _cut(world, name, {k: v[0] for k, v in world["alone"][name].items()})
            row = _cut(world, name, {k: v[r] for k, v in out.items()})
            for k in ALL:
                assert np.array_equal(a[k], row[k]), (name, k)


def test_rerun_graph_replay_and_output_subsets_give_the_same_bits(world):
    from ultrafnd_git_amd import audio
    group, x, lens, _ = world["batches"][0]
    first = audio.mel_spectrogram(x, lens, ALL)
    again = audio.mel_spectrogram(x, lens, ALL)
    for k in ALL:
        assert torch.equal(first[k], again[k]), k
    for want in (("mel_db",), ("mel_power",), ("mel_max",), ("mel_db", "mel_max"), ("mel_max", "mel_power")):
        sub = audio.mel_spectrogram(x, lens, want)
        assert tuple(sub) == tuple(k for k in ALL if k in want)      # what was not asked for is not stored
        for k in want:
            assert torch.equal(sub[k], first[k]), (want, k)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()      # a captured call, replayed on new content of the same buffers
    xs, ls = x.clone(), lens.clone()
    with torch.cuda.graph(graph):
        held = audio.mel_spectrogram(xs, ls, ALL)
    perm = list(range(1, len(group))) + [0]
    xs.copy_(x[perm])
    ls.copy_(lens[perm])
    graph.replay()
    torch.cuda.synchronize()
    for k in ALL:
        assert torch.equal(held[k], first[k][perm]), k


def test_the_class_routes_to_the_librosa_branch_and_matches_row_for_row(world):
    from ultrafnd_git_amd import audio
    gen = audio.MelSpectrogramGenerator(branch="librosa", max_batch=3)
    some = ["len1", "tone440", "len10240", "quiet_then_loud", "len161", "zeros", "len20479"]
    waves = [world["clips"][n] for n in some]
    flat, mats = gen.generate_batch(waves), gen.generate_batch(waves, flatten=False)
    for n, w, f, m in zip(some, waves, flat, mats):
        T = M.frame_counts(len(w))[0]
        want = world["alone"][n]["mel_db"][0][:, :T]
        assert m.shape == (64, T) and m.dtype == np.float32 and f.shape == (64 * T,)
        assert np.array_equal(m, want) and np.array_equal(f, want.flatten()), n
        assert np.array_equal(gen.generate(w), f) and np.array_equal(gen.generate(w, flatten=False), m), n


def test_the_default_branch_is_unchanged(world):
    from ultrafnd_git_amd import audio
    gen = audio.MelSpectrogramGenerator()
    for n in ("noise", "len10240", "len20480"):
        w = world["clips"][n]
        T = audio.stft_frame_count(len(w))
        want = audio.stft_forensics(torch.from_numpy(w)[None].to(DEV), None, want=("mel_like",))["mel_like"].cpu().numpy()[0][:, :T]
        assert np.array_equal(gen.generate(w, flatten=False), want) and np.array_equal(gen.generate(w), want.flatten()), n
        assert not np.array_equal(audio.MelSpectrogramGenerator(branch="librosa").generate(w, flatten=False), want), n
