"""CPU: the librosa-branch entries (csrc/spectral_desc.hip) and their Python layer (ultrafnd_git_amd/audio.py) refuse bad calls by
name without touching a GPU; the host-built basis is checked against the restatement's window and angles."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import librosa_ref as R

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch
REPO = Path(__file__).resolve().parents[1]


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def test_exported_constants_and_struct_mirror_the_header():
    from ultrafnd_git_amd import _lib as L
    text = (REPO / "include" / "ultrafnd_hip.h").read_text()
    assert int(re.search(r"#define UFND_DESC_FRAME_TILE_A (\d+)", text).group(1)) == L.DESC_FRAME_TILE_A == 64
    assert int(re.search(r"#define UFND_DESC_FRAME_TILE_B (\d+)", text).group(1)) == L.DESC_FRAME_TILE_B == 32
    members = re.search(r"typedef struct ufnd_spectral_desc_out \{(.*?)\}", text, flags=re.S).group(1)
    names = re.findall(r"\*(\w+)", members)
    assert names == [n for n, _ in L.SpectralDescOut._fields_] and ctypes.sizeof(L.SpectralDescOut) == 8 * len(names) == 88


def test_workspace_query_and_its_64_bit_size():
    lib = _lib()
    r16 = lambda n: -(-n // 16) * 16
    for B, n in ((1, 1), (1, 16000), (32, 80000), (7, 10241), (3, 1 << 30)):
        TA, TB = 1 + n // 160, 1 + n // 512
        want = (r16(B * -(-TA // 64) * 32) + 2 * r16(B * 7 * TA * 4) + r16(B * TA * 4) + 4 * r16(B * TB * 4)
                + r16(B * -(-TB // 32) * 32 * 1056 * 4))
        assert lib.ufnd_spectral_desc_workspace_bytes(B, n) == want, (B, n)
    assert lib.ufnd_spectral_desc_workspace_bytes(65535, 1 << 30) > 1 << 48       # a size_t, far past 2^32
    for B, n in ((0, 400), (-1, 400), (65536, 400), (1, 0), (1, (1 << 30) + 1)):
        assert lib.ufnd_spectral_desc_workspace_bytes(B, n) == 0, (B, n)


def test_descriptor_entry_refusals():
    from ultrafnd_git_amd import _lib as L
    lib = _lib()
    err = lib.ufnd_last_error

    def call(waves=P, ba=P, bb=P, ws=P, out="features", B=2, n_max=16000, dim=128):
        io = None if out is None else L.SpectralDescOut(**{k: P for k in ([out] if out else [])})
        return lib.ufnd_spectral_descriptors(waves, None, ba, bb, ws, io, B, n_max, dim, None)

    assert call(waves=None) == 1 and b"null" in err()
    assert call(ba=None) == 1 and b"null" in err()
    assert call(bb=None) == 1 and b"null" in err()
    assert call(ws=None) == 1 and b"null" in err()
    assert call(out=None) == 1 and b"null" in err()
    assert call(out="") == 1 and b"no output" in err()
    assert call(B=0) == 1 and b"B=0" in err()
    assert call(B=65536) == 1 and b"B=65536" in err()
    assert call(n_max=0) == 1 and b"n_max=0" in err()
    assert call(n_max=(1 << 30) + 1) == 1 and b"n_max=1073741825" in err()
    assert call(dim=0) == 1 and b"dim=0" in err()
    assert call(ba=P + 4) == 1 and b"alignment" in err()
    assert call(bb=P + 8) == 1 and b"alignment" in err()
    assert call(ws=P + 8) == 1 and b"alignment" in err()


def test_python_refusals_by_name():
    from ultrafnd_git_amd import audio
    from ultrafnd_git_amd._lib import UltrafndHipError
    wave = torch.zeros(2, 1000)
    with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
        audio.spectral_descriptors(wave)
    with pytest.raises(UltrafndHipError, match="HIP device only"):
        audio.cache_audio(wave, branch="librosa")
    with pytest.raises(UltrafndHipError, match="HIP device"):
        audio.spectral_descriptors(np.zeros((2, 1000), np.float32))
    with pytest.raises(TypeError, match="hash"):
        audio.spectral_descriptors("a title")
    with pytest.raises(ValueError, match="pad_mode='reflect'"):
        audio.spectral_descriptors(wave, pad_mode="reflect")
    with pytest.raises(ValueError, match="want='mel_db'"):
        audio.spectral_descriptors(wave, want=("mel_db",))
    with pytest.raises(ValueError, match="want is empty"):
        audio.spectral_descriptors(wave, want=())
    with pytest.raises(ValueError, match="dim=0"):
        audio.spectral_descriptors(wave, dim=0)
    with pytest.raises(ValueError, match="branch='fft'"):
        audio.cache_audio(wave, branch="fft")
    with pytest.raises(ValueError, match="branch='fft'"):
        audio.VoiceCloneDetector(branch="fft")
    with pytest.raises(ValueError, match="branch='pyin'"):
        audio.SpectralForensics(branch="pyin")
    with pytest.raises(ValueError, match="n_fft=512"):
        audio.spectral_basis(512)


def test_librosa_branch_builds_no_encoder_and_keeps_the_defaults():
    from ultrafnd_git_amd import audio
    sf = audio.SpectralForensics(branch="librosa")
    assert sf.encoder is None and sf.dim == 128 and sf.branch == "librosa"
    with pytest.raises(ValueError, match="encoder=None"):
        audio.SpectralForensics(branch="librosa", encoder=object())
    with pytest.raises(TypeError, match="hash"):
        sf.extract("a title")
    with pytest.raises(ValueError, match="sr=8000"):
        sf.extract(np.zeros(1000, np.float32), sr=8000)
    with pytest.raises(ValueError, match="clip length 0"):
        sf.extract_batch([np.zeros(1000, np.float32), np.zeros(0, np.float32)])
    assert audio.VoiceCloneDetector().branch == "energy" and audio.VoiceCloneDetector(branch="librosa").branch == "librosa"
    import inspect
    assert inspect.signature(audio.cache_audio).parameters["branch"].default == "stft"
    assert inspect.signature(audio.SpectralForensics.__init__).parameters["branch"].default == "w2v2"


@pytest.mark.parametrize("n_fft", [400, 2048])
def test_spectral_basis_is_the_window_folded_dft_rounded_once(n_fft):
    from ultrafnd_git_amd import audio
    b = audio.spectral_basis(n_fft)
    bins = n_fft // 2 + 1
    assert b.shape == (2 * bins, n_fft) and b.dtype == np.float32
    rng = np.random.default_rng(n_fft)
    x = rng.standard_normal(n_fft)
    spec = np.fft.rfft(x * R.window(n_fft))
    mine = b.astype(np.float64) @ x
    scale = np.abs(x).sum()
    assert np.abs(mine[:bins] - spec.real).max() <= 2 * R.U * scale and np.abs(mine[bins:] - spec.imag).max() <= 2 * R.U * scale
    assert not b[:, 0].any() and not b[bins].any()      # w[0] = 0; sin of bin 0
    assert audio.desc_frame_counts(0) == (0, 0) and audio.desc_frame_counts(1) == (1, 1) and audio.desc_frame_counts(10240) == (65, 21)
