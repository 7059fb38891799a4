"""The audio encoder (ultrafnd_git_amd/audio.py) against the float64 yardstick of tests/audio_ref.py: the installed
transformers.Wav2Vec2Model in float64, one clip at a time.

Bounds: for every bf16 stage and for the features, each of the three criteria (max-abs, relative L2, 1 - cosine) is held to
3 x the bf16-operand mirror's own error against float64 ON THAT SAME INPUT (audio_ref.bounds_from_mirror), computed here on the
CPU; fp32-only stages (normalisation, conv0 + GroupNorm before its bf16 rounding, mean-pool, projection) to the rounding bounds of
audio_ref.FP32_BOUNDS.  Every test prints its figures before it asserts; tools/audio_errors.py collects them.
"""
import numpy as np
import pytest
import torch

from tests import audio_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS, MIXED = R.LENGTHS, R.MIXED      # (tests/audio_ref.py says what each length exercises)


class _Case:
    """An encoder, its weights, and per-clip float64 reference / mirror results computed once and shared."""

    def __init__(self, layers, scale_channel=None):
        from ultrafnd_git_amd.audio import Wav2Vec2AudioEncoder
        self.layers = layers
        self.enc = Wav2Vec2AudioEncoder(layers=layers)
        self.enc.load_state_dict(R.case_weights(self.enc.state_dict(), scale_channel))
        self.sd = self.enc.state_dict()
        self.enc = self.enc.to(DEV)
        self.model = R.hf_model(self.sd, layers)
        self._waves, self._ref, self._mir = {}, {}, {}

    def wave(self, n):
        if n not in self._waves:
            self._waves[n] = R.make_waves([n], seed=n)[0]
        return self._waves[n]

    def ref(self, n):
        if n not in self._ref:
            self._ref[n] = R.reference(self.sd, self.wave(n), self.layers, model=self.model)
        return self._ref[n]

    def mir(self, n):
        if n not in self._mir:
            self._mir[n] = R.mirror(self.sd, self.wave(n), self.layers)
        return self._mir[n]


@pytest.fixture(scope="module")
def case2():
    return _Case(2)


def _hold(name, got, ref, mir):
    """got within 3 x the mirror's own error of the float64 reference, on each criterion."""
    c, b = R.criteria(got.double().cpu(), ref), R.bounds_from_mirror(mir, ref)
    for k in c:
        print(f"AUDIO_ERR {name} {k} gpu={c[k]:.3e} bound={b[k]:.3e} ratio_to_mirror={R.BOUND_FACTOR * c[k] / b[k]:.2f}")
    bad = {k: (c[k], b[k]) for k in c if not c[k] <= b[k]}
    assert not bad, (name, bad)


def _hold_fp32(name, got, ref, rel, scale=None):
    ref = torch.as_tensor(ref).double()
    s = float(ref.abs().max()) if scale is None else float(scale)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"AUDIO_ERR {name} max_abs gpu={err:.3e} bound={rel * max(s, 1e-30):.3e} ratio_to_bound={err / (rel * max(s, 1e-30)):.2f}")
    assert err <= rel * s, (name, err, rel * s)


@pytest.mark.parametrize("n", LENGTHS)
def test_stages_against_float64(case2, n):
    c, enc = case2, case2.enc
    w = c.wave(n)[None]
    ref, mir = c.ref(n), c.mir(n)
    assert ref["pos"].shape[0] == enc.last_hidden_state(w, stage="pos")[0].shape[0] == R.frame_counts(n)[-1]
    _hold_fp32(f"n{n}.norm", enc.normalized(w)[0], ref["norm"], R.FP32_BOUNDS["norm"])
    _hold_fp32(f"n{n}.conv0", enc.last_hidden_state(w, stage="conv0")[0], ref["conv0"], R.FP32_BOUNDS["conv0"])
    _hold(f"n{n}.conv", enc.last_hidden_state(w, stage="conv")[0], ref["conv"], mir["conv"])
    _hold(f"n{n}.pos", enc.last_hidden_state(w, stage="pos")[0], ref["pos"], mir["pos"])
    for i in (1, 2):
        _hold(f"n{n}.layer{i}", enc.last_hidden_state(w, n_layers=i)[0], ref["layers"][i - 1], mir["layers"][i - 1])
    _hold(f"n{n}.feature", enc(w)[0], ref["feature"], mir["feature"])


def test_pool_and_projection_are_fp32_exact(case2):
    """The mean over a clip's frames and the 768 -> 128 projection, against float64 ON THE GPU'S OWN hidden state."""
    c, enc = case2, case2.enc
    for n in (400, 16000, 41680):
        w = c.wave(n)[None]
        h = enc.last_hidden_state(w)[0].double().cpu()
        feat = enc(w)[0].clone()
        pooled = enc.pooled(w)[0]
        _hold_fp32(f"n{n}.pool", pooled, h.mean(dim=0), R.FP32_BOUNDS["pool"], scale=h.abs().max())
        pw, pb = c.sd["proj.weight"].double(), c.sd["proj.bias"].double()
        x = pooled.double().cpu()
        scale = float(((pw.abs() * x.abs()[None]).sum(1) + pb.abs()).max())
        _hold_fp32(f"n{n}.proj", feat, pw @ x + pb, R.FP32_BOUNDS["proj"], scale=scale)


def _mixed_batch(c, garbage):
    n_max = max(MIXED)
    batch = torch.full((len(MIXED), n_max), garbage, dtype=torch.float32)
    if garbage != 0.0:      # nonzero garbage beyond each clip: nothing valid may read it
        batch = batch * torch.randn(len(MIXED), n_max, generator=torch.Generator().manual_seed(3))
    for r, n in enumerate(MIXED):
        batch[r, :n] = c.wave(n)
    return batch


def test_mixed_batch_is_bit_identical_to_single_clips(case2):
    c, enc = case2, case2.enc
    batch = _mixed_batch(c, 1e3)
    f1 = enc(batch, list(MIXED)).clone()
    hs = [t.clone() for t in enc.last_hidden_state(batch, list(MIXED))]
    f2 = enc(batch, list(MIXED)).clone()
    assert torch.equal(f1, f2), "two runs differ"
    assert torch.isfinite(f1).all()
    for r, n in enumerate(MIXED):
        alone = enc(c.wave(n)[None]).clone()
        h_alone = enc.last_hidden_state(c.wave(n)[None])[0]
        print(f"AUDIO_BITS n{n} hidden_equal={torch.equal(hs[r], h_alone)} feature_equal={torch.equal(f1[r], alone[0])} "
              f"max_diff={(f1[r] - alone[0]).abs().max().item():.3e}")
        assert torch.equal(hs[r], h_alone), f"clip of {n} samples: hidden state differs between the batch and alone"
        assert torch.equal(f1[r], alone[0]), f"clip of {n} samples: feature differs between the batch and alone"
        _hold(f"mixed.n{n}.feature", f1[r], c.ref(n)["feature"], c.mir(n)["feature"])
    # the same clips with a different batch composition and padding content
    f3 = enc(_mixed_batch(c, 0.0)[[3, 1]], [MIXED[3], MIXED[1]]).clone()
    assert torch.equal(f3[0], f1[3]) and torch.equal(f3[1], f1[1])


def test_outlier_channel_keeps_the_bounds():
    """One conv0 channel's weight scaled 20 x: GroupNorm takes the scale out again, and its statistics must do so at fp32 accuracy."""
    c = _Case(2, scale_channel=R.OUTLIER_CHANNEL)
    for n in R.OUTLIER_LENGTHS:
        w, ref, mir = c.wave(n)[None], c.ref(n), c.mir(n)
        _hold_fp32(f"outlier.n{n}.conv0", c.enc.last_hidden_state(w, stage="conv0")[0], ref["conv0"], R.FP32_BOUNDS["conv0"])
        _hold(f"outlier.n{n}.conv", c.enc.last_hidden_state(w, stage="conv")[0], ref["conv"], mir["conv"])
        _hold(f"outlier.n{n}.layer2", c.enc.last_hidden_state(w)[0], ref["layers"][1], mir["layers"][1])
        _hold(f"outlier.n{n}.feature", c.enc(w)[0], ref["feature"], mir["feature"])


def test_full_depth_features():
    c = _Case(12)
    lens = (16000, 16000)
    waves = torch.stack([R.make_waves([16000], seed=sd)[0] for sd in R.FULL_DEPTH_SEEDS])
    feat = c.enc(waves).clone()
    assert feat.shape == (2, 128) and feat.dtype == torch.float32
    for i, n in enumerate(lens):
        ref = R.reference(c.sd, waves[i], 12, model=c.model)
        mir = R.mirror(c.sd, waves[i], 12)
        assert not R.mirror_within_sanity(mir["feature"], ref["feature"])
        _hold(f"full12.clip{i}.feature", feat[i], ref["feature"], mir["feature"])


def test_spectral_forensics(case2):
    from ultrafnd_git_amd.audio import SpectralForensics
    sf = SpectralForensics(dim=128, encoder=case2.enc, max_batch=3)
    g = torch.Generator().manual_seed(11)
    stereo = (0.1 * torch.randn(2, 3000, generator=g)).numpy()
    a = sf.extract(stereo)
    assert a.shape == (128,) and a.dtype == np.float32
    assert np.array_equal(a, sf.extract(stereo.mean(axis=0))), "stereo is mono-mixed as the reference does"
    assert np.array_equal(a, sf.extract(torch.from_numpy(stereo)))
    with pytest.raises(TypeError, match="hash"):
        sf.extract("some title text")
    with pytest.raises(ValueError, match="sr=8000"):
        sf.extract(stereo, sr=8000)
    clips = [case2.wave(n).numpy() for n in (1040, 400, 16000, 720)] + [stereo]
    out = sf.extract_batch(clips)
    assert out.shape == (5, 128)
    for i, clip in enumerate(clips):
        assert np.array_equal(out[i], sf.extract(clip)), f"extract_batch row {i} differs from extract"


def test_refusals_on_the_device(case2):
    enc = case2.enc
    with pytest.raises(ValueError, match="at least 400"):
        enc(torch.zeros(1, 399))
    with pytest.raises(ValueError, match="at least 400"):
        enc(torch.zeros(2, 1000), [1000, 399])
    with pytest.raises(ValueError, match="n_max"):
        enc(torch.zeros(1, 1000), [1001])


def test_work_buffers_do_not_grow_with_the_number_of_distinct_lengths(case2):
    """A cache builder sees a new clip length with almost every group: the work buffers are those of the largest pass, however
    many lengths went through, and a clip's feature does not depend on what the buffers held before."""
    c, enc = case2, case2.enc
    big = c.wave(41680)[None]
    first = enc(big).clone()
    names, held = set(enc._bufs), enc.workspace_bytes()
    g = torch.Generator().manual_seed(5)
    small = {}
    for n in [400 + 97 * i for i in range(40)]:      # 40 distinct lengths, alone and in pairs
        w = 0.1 * torch.randn(2, n, generator=g)
        small[n] = enc(w, [n, n - 3 if n > 403 else n]).clone()
        assert torch.equal(enc(w[:1]).clone()[0], small[n][0])
    assert set(enc._bufs) == names and enc.workspace_bytes() == held, (enc.workspace_bytes(), held)
    assert torch.equal(enc(big), first)
    assert held < 2 * 1024 ** 3
