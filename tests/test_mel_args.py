"""CPU: the mel-dB entries (csrc/mel_db.hip) and their Python layer (ultrafnd_git_amd/audio.py) refuse bad calls by name without
touching a GPU; MelSpectrogramGenerator's defaults and messages are what they were."""
import inspect
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
    assert int(re.search(r"#define UFND_MEL_FRAME_TILE (\d+)", text).group(1)) == L.MEL_FRAME_TILE == 64
    assert int(re.search(r"#define UFND_MEL_FILTERS (\d+)", text).group(1)) == L.MEL_FILTERS == 64
    assert int(re.search(r"#define UFND_MEL_NNZ (\d+)", text).group(1)) == L.MEL_NNZ == 388
    assert "size_t ufnd_mel_workspace_bytes(int B, int n_max);" in text and "int ufnd_mel_spectrogram(const float* waves" in text


def test_workspace_query_and_its_64_bit_size():
    lib = _lib()
    r16 = lambda n: -(-n // 16) * 16
    for B, n in ((1, 1), (1, 16000), (32, 80000), (7, 10241), (3, 1 << 30), (65535, 1 << 30)):
        T = 1 + n // 160
        assert lib.ufnd_mel_workspace_bytes(B, n) == r16(B * 64 * T * 4) + r16(B * -(-T // 64) * 4), (B, n)
    assert lib.ufnd_mel_workspace_bytes(3, 1 << 30) > 1 << 32       # a size_t, past 2^32
    for B, n in ((0, 400), (-1, 400), (65536, 400), (1, 0), (1, -5), (1, (1 << 30) + 1)):
        assert lib.ufnd_mel_workspace_bytes(B, n) == 0, (B, n)


def test_mel_entry_refusals():
    lib = _lib()
    err = lib.ufnd_last_error

    def call(waves=P, basis=P, w=P, first=P, count=P, ws=P, outs=(P, None, None), B=2, n_max=16000):
        return lib.ufnd_mel_spectrogram(waves, None, basis, w, first, count, ws, outs[0], outs[1], outs[2], B, n_max, None)

    for key in ("waves", "basis", "w", "first", "count", "ws"):
        assert call(**{key: None}) == 1 and b"null" in err(), key
    assert call(outs=(None, None, None)) == 1 and b"no output" in err()
    assert call(B=0) == 1 and b"B=0" in err()
    assert call(B=65536) == 1 and b"B=65536" in err()
    assert call(n_max=0) == 1 and b"n_max=0" in err()
    assert call(n_max=(1 << 30) + 1) == 1 and b"n_max=1073741825" in err()
    assert call(basis=P + 4) == 1 and b"alignment" in err()
    assert call(ws=P + 8) == 1 and b"alignment" in err()
    assert call(w=P + 2) == 1 and b"alignment" in err()
    assert call(first=P + 1) == 1 and b"alignment" in err()
    assert call(count=P + 3) == 1 and b"alignment" in err()


def test_python_refusals_by_name():
    from ultrafnd_git_amd import audio
    from ultrafnd_git_amd._lib import UltrafndHipError
    wave = torch.zeros(2, 1000)
    with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
        audio.mel_spectrogram(wave)
    with pytest.raises(UltrafndHipError, match="HIP device"):
        audio.mel_spectrogram(np.zeros((2, 1000), np.float32))
    with pytest.raises(TypeError, match="hash"):
        audio.mel_spectrogram("a title")
    with pytest.raises(ValueError, match="want='magnitude'"):
        audio.mel_spectrogram(wave, want=("magnitude",))
    with pytest.raises(ValueError, match="want='mel_like'"):
        audio.mel_spectrogram(wave, want=("mel_db", "mel_like"))
    with pytest.raises(ValueError, match="want is empty"):
        audio.mel_spectrogram(wave, want=())
    for kw, msg in ((dict(n_mels=128), "n_mels=128"), (dict(n_fft=512), "n_fft=512"), (dict(hop_length=200), "hop_length=200"), (dict(sr=22050), "sr=22050"),
                    (dict(branch="htk"), "branch='htk'"), (dict(branch="stft"), "branch='stft'"), (dict(htk=True), "htk=True"),
                    (dict(norm=None), "norm=None"), (dict(norm=1), "norm=1"), (dict(pad_mode="reflect"), "pad_mode='reflect'")):
        for branch in ({}, {"branch": "librosa"}):
            with pytest.raises(ValueError, match=re.escape(msg)):
                audio.MelSpectrogramGenerator(**{**branch, **kw})


def test_generator_defaults_and_messages_are_unchanged():
    from ultrafnd_git_amd import audio
    sig = inspect.signature(audio.MelSpectrogramGenerator.__init__).parameters
    assert [sig[k].default for k in ("sr", "n_mels", "n_fft", "hop_length", "max_batch", "resample", "branch")] == [16000, 64, 400, 160, 32, None, "torch"]
    g = audio.MelSpectrogramGenerator()
    assert (g.branch, g.sr, g.n_mels, g.n_fft, g.hop, g.resample) == ("torch", 16000, 64, 400, 160, None)
    with pytest.raises(ValueError, match=r"n_mels=80: MelSpectrogramGenerator is built for the reference's defaults \(n_mels=64\)"):
        audio.MelSpectrogramGenerator(n_mels=80)
    with pytest.raises(ValueError, match="clip length 200: the STFT branch needs at least 201 samples"):      # the default keeps torch.stft's rule
        g.generate(np.zeros(200, np.float32))
    with pytest.raises(ValueError, match="sr=8000: MelSpectrogramGenerator takes 16 kHz audio"):
        g.generate(np.zeros(1000, np.float32), sr=8000)
    with pytest.raises(TypeError, match="hash"):
        g.generate("a title")
    lib = audio.MelSpectrogramGenerator(branch="librosa", resample="kaiser_fast")
    assert (lib.branch, lib.resample) == ("librosa", "kaiser_fast")
    with pytest.raises(ValueError, match="clip length 0: the librosa branch needs at least one sample"):
        audio.MelSpectrogramGenerator(branch="librosa").generate_batch([np.zeros(10, np.float32), np.zeros(0, np.float32)])
    with pytest.raises(ValueError, match="resample='best'"):
        audio.MelSpectrogramGenerator(branch="librosa", resample="best")
