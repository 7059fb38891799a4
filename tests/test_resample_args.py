"""CPU: the resampler's entry (csrc/resample.hip) and its Python layer (ultrafnd_git_amd/audio.py) refuse bad calls by name without
touching a GPU, and the classes keep refusing anything but 16 kHz audio unless they are given a `resample` quality."""
import numpy as np
import pytest
import torch

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch


def test_classes_without_a_resample_quality_refuse_other_rates_with_the_present_messages():
    from ultrafnd_git_amd import audio
    sf = audio.SpectralForensics(branch="stft")
    mel, clone = audio.MelSpectrogramGenerator(), audio.VoiceCloneDetector()
    assert sf.resample is None and mel.resample is None and clone.resample is None
    x = np.zeros(1000, np.float32)
    tail = r"takes 16 kHz audio \(the reference resamples with librosa, which is not part of this package\)"
    with pytest.raises(ValueError, match=r"sr=8000: SpectralForensics " + tail):
        sf.extract(x, sr=8000)
    with pytest.raises(ValueError, match=r"sr=22050: SpectralForensics " + tail):
        sf.extract_batch([x, x], sr=22050)
    with pytest.raises(ValueError, match=r"sr=22050: MelSpectrogramGenerator " + tail):
        mel.generate(x, sr=22050)
    with pytest.raises(ValueError, match=r"sr=44100: MelSpectrogramGenerator " + tail):
        mel.generate_batch([x], sr=44100)
    with pytest.raises(ValueError, match=r"sr=8000: VoiceCloneDetector " + tail):
        clone.score(x, sr=8000)
    with pytest.raises(ValueError, match=r"sr=48000: VoiceCloneDetector " + tail):
        clone.score_batch([x], sr=48000)
    with pytest.raises(ValueError, match=r"sr=8000: SpectralForensics " + tail):
        audio.SpectralForensics._mono_16k(x, 8000)
    assert audio.SpectralForensics(device="cpu").resample is None      # the default (w2v2) branch too


def test_resample_keyword_of_the_classes():
    from ultrafnd_git_amd import audio
    for q in audio.RESAMPLE_QUALITIES:
        assert audio.SpectralForensics(branch="stft", resample=q).resample == q
        assert audio.MelSpectrogramGenerator(resample=q).resample == q
        assert audio.VoiceCloneDetector(resample=q).resample == q
    for make, who in ((lambda **k: audio.SpectralForensics(branch="stft", **k), "SpectralForensics"),
                      (audio.MelSpectrogramGenerator, "MelSpectrogramGenerator"), (audio.VoiceCloneDetector, "VoiceCloneDetector")):
        for bad in ("soxr_hq", "", True, 3):
            with pytest.raises(ValueError, match=rf"resample=.*{who} takes None .*kaiser_best.*kaiser_fast.*hann"):
                make(resample=bad)
    sf = audio.SpectralForensics(branch="stft", resample="hann")
    x = np.zeros(1000, np.float32)
    with pytest.raises(ValueError, match="positive integer"):      # rates are checked before anything runs
        sf.extract(x, sr=0)
    with pytest.raises(ValueError, match="above 1024"):
        sf.extract(x, sr=44101)
    with pytest.raises(ValueError, match="2 rates for 1 clips"):
        sf.extract_batch([x], sr=[44100, 48000])
    with pytest.raises(TypeError, match="hash"):
        sf.extract("a title", sr=44100)
    with pytest.raises(ValueError, match=r"expected \(T,\) or \(C, T\)"):
        sf.extract(np.zeros((2, 2, 50), np.float32), sr=44100)


def test_resample_refusals_by_name():
    from ultrafnd_git_amd import audio
    from ultrafnd_git_amd._lib import UltrafndHipError
    wave = torch.zeros(2, 1000)
    with pytest.raises(ValueError, match="orig_sr is required"):
        audio.resample(wave)
    with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
        audio.resample(wave, orig_sr=44100)
    with pytest.raises(UltrafndHipError, match="HIP device"):
        audio.resample(np.zeros((2, 1000), np.float32), orig_sr=44100)
    with pytest.raises(UltrafndHipError, match="HIP device"):
        audio.resample("a title", orig_sr=44100)
    with pytest.raises(ValueError, match="quality='best'"):
        audio.resample(wave, orig_sr=44100, quality="best")
    with pytest.raises(ValueError, match="positive integer"):
        audio.resample(wave, orig_sr=44100, new_sr=0)
    with pytest.raises(ValueError, match="above 1024"):
        audio.resample(wave, orig_sr=16000, new_sr=44101)
    meta = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="meta")
    with pytest.raises(UltrafndHipError, match="HIP device only"):
        audio.resample(meta(2, 1000), orig_sr=44100)
    # cache_audio: the default path is untouched; the new keywords are checked by name
    with pytest.raises(UltrafndHipError, match="HIP device only"):
        audio.cache_audio(wave, sr=44100)
    with pytest.raises(ValueError, match="positive integer"):
        audio.cache_audio(wave, sr=-1)
    with pytest.raises(ValueError, match="quality='soxr_hq'"):
        audio.cache_audio(wave, sr=44100, resample="soxr_hq")
    with pytest.raises(UltrafndHipError, match="HIP device only"):      # at 16 kHz the quality is not consulted: today's path
        audio.cache_audio(wave, sr=16000, resample="soxr_hq")


def test_entry_refusals():
    from ultrafnd_git_amd import _lib as L
    lib = L.lib()
    err = lib.ufnd_last_error

    def call(waves=P, dtype=0, sb=1000, sc=0, ss=1, taps=P, groups=P, out=P, out_lengths=P, B=2, C=1, n_max=1000, o=441, n=160, G=1, width=187,
             ngroups=40, tap_rows=15504, qt=64, kc=816, nchunks=1, scale=1.0):
        return lib.ufnd_resample(waves, dtype, sb, sc, ss, None, taps, groups, out, out_lengths, B, C, n_max, o, n, G, width, ngroups, tap_rows, qt, kc,
                                 nchunks, scale, None)

    for name in ("waves", "taps", "groups", "out", "out_lengths"):
        assert call(**{name: None}) == 1 and b"null" in err(), name
    assert call(dtype=2) == 1 and b"dtype=2" in err()
    assert call(B=0) == 1 and b"B=0" in err()
    assert call(B=65536) == 1 and b"B=65536" in err()
    assert call(C=0) == 1 and b"C=0" in err()
    assert call(C=65) == 1 and b"C=65" in err()
    assert call(n_max=0) == 1 and b"n_max=0" in err()
    assert call(n_max=(1 << 30) + 1) == 1 and b"n_max=1073741825" in err()
    assert call(o=0) == 1 and b"o=0" in err() and b"1024" in err()
    assert call(o=1025) == 1 and b"o=1025" in err() and b"1024" in err()
    assert call(n=1025, ngroups=257) == 1 and b"n=1025" in err()
    assert call(ss=-1) == 1 and b"negative stride" in err()
    assert call(G=0) == 1 and b"G=0" in err()
    assert call(ngroups=39) == 1 and b"ngroups=39" in err()
    assert call(width=-1) == 1 and b"width=-1" in err()
    assert call(qt=0) == 1 and b"qt=0" in err()
    assert call(qt=65) == 1 and b"qt=65" in err()
    assert call(kc=812) == 1 and b"kc=812" in err() and b"multiple of 8" in err()
    assert call(kc=40000) == 1 and b"40000" in err()      # 63 x 441 + kc floats must fit LDS
    assert call(nchunks=0) == 1 and b"nchunks=0" in err()
    assert call(o=1, n=1024, ngroups=256, n_max=1 << 30) == 1 and b"output samples per clip" in err()      # m_max = 2^40
    assert call(taps=P + 4) == 1 and b"alignment" in err()
    assert call(waves=P + 2) == 1 and b"alignment" in err()
    assert call(waves=P + 1, dtype=1) == 1 and b"alignment" in err()


def test_offsets_of_the_largest_accepted_call_fit_64_bits():
    """Input offsets b stride_b + c stride_c + s stride_s and output offsets b m_max + j are 64-bit in the kernel; at the accepted
    limits they pass 2^32 and stay below 2^63, and the in-tile terms fit an int."""
    from pathlib import Path
    from ultrafnd_git_amd import _lib as L
    B, C, n_max, m_max = 65535, 64, 1 << 30, (1 << 31) - 1
    assert B * C * n_max > 1 << 32 and B * C * n_max < 1 << 63 and B * m_max < 1 << 63
    assert (L.RESAMPLE_OUT_TILE - 1) * (1 << 20) < 1 << 31 and L.RESAMPLE_OUT_TILE * 65536 < 1 << 31
    src = (Path(__file__).resolve().parents[1] / "ultrafnd_git_amd" / "csrc" / "resample.hip").read_text()
    for expr in ("(long long)b * a.sb", "x + s * a.ss", "(size_t)b * (size_t)a.m_max", "(long long)tile * a.qt", "(long long)a.n * len + a.o - 1"):
        assert expr in src, expr
