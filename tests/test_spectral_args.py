"""CPU: the STFT audio forensics entries (csrc/spectral.hip) and their Python layer (ultrafnd_git_amd/audio.py) refuse bad calls
by name without touching a GPU; the 64-bit offset arithmetic of the entries is checked on the host."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch
REPO = Path(__file__).resolve().parents[1]


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def test_exported_constants_mirror_the_header():
    from ultrafnd_git_amd import _lib as L
    text = (REPO / "include" / "ultrafnd_hip.h").read_text()
    assert int(re.search(r"#define UFND_STFT_FRAME_TILE (\d+)", text).group(1)) == L.STFT_FRAME_TILE
    assert int(re.search(r"#define UFND_STFT_MIN_SAMPLES (\d+)", text).group(1)) == L.STFT_MIN_SAMPLES == 201
    assert L.STFT_FRAME_TILE % 32 == 0


def test_workspace_query_and_its_64_bit_size():
    from ultrafnd_git_amd import _lib as L
    lib, ft = _lib(), L.STFT_FRAME_TILE
    tiles = lambda n: -(-(1 + n // 160) // ft)
    for B, n in ((1, 201), (1, 16000), (32, 80000), (7, 10080), (3, 1 << 30), (65535, 1 << 30)):
        assert lib.ufnd_spectral_workspace_bytes(B, n) == B * tiles(n) * 32, (B, n)
    assert lib.ufnd_spectral_workspace_bytes(65535, 1 << 30) > 1 << 37       # a size_t, far past 2^31
    for B, n in ((0, 400), (-1, 400), (65536, 400), (1, 0), (1, (1 << 30) + 1)):
        assert lib.ufnd_spectral_workspace_bytes(B, n) == 0, (B, n)


def test_offsets_of_the_largest_accepted_call_need_and_fit_64_bits():
    """The kernels index waves at b n_max + i, magnitude at (b 201 + bin) T_max + t and mel_like at (b 64 + band) T_max + t in size_t.
    At the limits the entries accept these pass 2^31 and 2^32 (so 32-bit arithmetic would be wrong) and stay far below 2^63; the
    in-clip terms (a mirrored sample index up to 2 (len - 1), a padded index up to len + 399, a frame index) fit an int."""
    B, n_max = 65535, 1 << 30
    T_max = 1 + n_max // 160
    assert (B - 1) * n_max + n_max - 1 > 1 << 32 and (B - 1) * n_max + n_max < 1 << 63
    assert ((B - 1) * 201 + 200) * T_max + T_max - 1 > 1 << 32 and B * 201 * T_max < 1 << 63
    assert 2 * (n_max - 1) < 1 << 31 and n_max + 399 < 1 << 31 and T_max * 160 + 64 * 160 + 400 < 1 << 31
    src = (REPO / "ultrafnd_git_amd" / "csrc" / "spectral.hip").read_text()
    for expr in ("(size_t)b * n_max", "(size_t)b * BINS * T_max", "(size_t)b * BANDS * T_max", "(size_t)bin * T_max", "(size_t)m * T_max",
                 "(size_t)b * tiles_max + tile", "(size_t)b * dim"):
        assert expr in src, expr


def test_stft_forensics_refusals():
    lib = _lib()
    err = lib.ufnd_last_error

    def call(waves=P, basis=P, ws=P, mag=None, mel=None, stats=P, feats=P, B=2, n_max=16000, dim=128):
        return lib.ufnd_stft_forensics(waves, None, basis, ws, mag, mel, stats, feats, B, n_max, dim, None)

    assert call(waves=None) == 1 and b"null" in err()
    assert call(basis=None) == 1 and b"null" in err()
    assert call(stats=None, feats=None) == 1 and b"no output" in err()
    assert call(B=0) == 1 and b"B=0" in err()
    assert call(B=65536) == 1 and b"B=65536" in err()
    assert call(n_max=0) == 1 and b"n_max=0" in err()
    assert call(n_max=(1 << 30) + 1) == 1 and b"n_max=1073741825" in err()
    assert call(ws=None) == 1 and b"workspace" in err()
    assert call(dim=0) == 1 and b"dim=0" in err()
    assert call(dim=-4) == 1 and b"dim=-4" in err()
    assert call(basis=P + 4) == 1 and b"alignment" in err()
    assert call(ws=P + 4) == 1 and b"alignment" in err()


def test_wave_energy_refusals():
    lib = _lib()
    err = lib.ufnd_last_error
    assert lib.ufnd_wave_energy(None, None, P, P, 1, 400, None) == 1 and b"null" in err()
    assert lib.ufnd_wave_energy(P, None, None, None, 1, 400, None) == 1 and b"null" in err()
    assert lib.ufnd_wave_energy(P, None, P, P, 0, 400, None) == 1 and b"B=0" in err()
    assert lib.ufnd_wave_energy(P, None, P, P, 1, 0, None) == 1 and b"n_max=0" in err()


def test_python_refusals_by_name():
    from ultrafnd_git_amd import audio
    from ultrafnd_git_amd._lib import UltrafndHipError
    wave = torch.zeros(2, 1000)
    for call in (audio.stft_forensics, audio.cache_audio, audio.wave_energy):
        with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
            call(wave)
        with pytest.raises(TypeError, match="hash"):
            call("a title")
        with pytest.raises(UltrafndHipError, match="HIP device"):
            call(np.zeros((2, 1000), np.float32))
    with pytest.raises(ValueError, match="want='phase'"):
        audio.stft_forensics(wave, want=("phase",))
    with pytest.raises(ValueError, match="want is empty"):
        audio.stft_forensics(wave, want=())
    with pytest.raises(ValueError, match="dim=0"):
        audio.stft_forensics(wave, dim=0)
    meta = torch.empty(2, 1000, device="meta")
    with pytest.raises(UltrafndHipError, match="HIP device only"):
        audio.stft_forensics(meta)


def test_stft_branch_builds_no_encoder_and_refuses_what_the_reference_cannot_reproduce():
    from ultrafnd_git_amd import audio
    sf = audio.SpectralForensics(branch="stft")
    assert sf.encoder is None and sf.dim == 128 and sf.branch == "stft"
    with pytest.raises(TypeError, match="hash"):
        sf.extract("a title")
    with pytest.raises(ValueError, match="sr=8000"):
        sf.extract(np.zeros(1000, np.float32), sr=8000)
    with pytest.raises(ValueError, match="clip length 200"):
        sf.extract(np.zeros(200, np.float32))
    with pytest.raises(ValueError, match="clip length 7"):
        sf.extract_batch([np.zeros(1000, np.float32), np.zeros(7, np.float32)])
    with pytest.raises(ValueError, match="branch='fft'"):
        audio.SpectralForensics(branch="fft")
    with pytest.raises(ValueError, match="dim=0"):
        audio.SpectralForensics(dim=0, branch="stft")
    with pytest.raises(ValueError, match="encoder=None"):
        audio.SpectralForensics(branch="stft", encoder=object())


def test_default_spectral_forensics_still_builds_the_encoder():
    from ultrafnd_git_amd import audio
    sf = audio.SpectralForensics(device="cpu")
    assert sf.branch == "w2v2" and isinstance(sf.encoder, audio.Wav2Vec2AudioEncoder) and sf.encoder.out_dim == 128


def test_mel_generator_and_clone_detector_refusals():
    from ultrafnd_git_amd import audio
    for kw, name in ((dict(sr=8000), "sr=8000"), (dict(n_mels=80), "n_mels=80"), (dict(n_fft=512), "n_fft=512"), (dict(hop_length=200), "hop_length=200")):
        with pytest.raises(ValueError, match=name):
            audio.MelSpectrogramGenerator(**kw)
    mel, clone = audio.MelSpectrogramGenerator(), audio.VoiceCloneDetector()
    assert (mel.sr, mel.n_mels, mel.n_fft, mel.hop) == (16000, 64, 400, 160)
    with pytest.raises(TypeError, match="hash"):
        mel.generate("a title")
    with pytest.raises(ValueError, match="sr=22050"):
        mel.generate(np.zeros(1000, np.float32), sr=22050)
    with pytest.raises(ValueError, match="clip length 100"):
        mel.generate(np.zeros(100, np.float32))
    with pytest.raises(TypeError, match="hash"):
        clone.score("a title")
    with pytest.raises(ValueError, match="sr=8000"):
        clone.score(np.zeros(1000, np.float32), sr=8000)
