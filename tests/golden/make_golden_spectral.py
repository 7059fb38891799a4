#!/usr/bin/env python3
"""Mint tests/golden/spectral.npz from the REAL reference's SpectralForensics, MelSpectrogramGenerator and VoiceCloneDetector
(src/core_blocks/audio_blocks.py).

Needs a checkout of the reference project (it is not part of this repository and never travels with it):

    python tests/golden/make_golden_spectral.py <path to the reference checkout>

`transformers` and `librosa` are masked before the import, so the module takes the branches it takes on a host without a wav2vec2
checkpoint and without librosa (asserted: _HAS_W2V2 and _HAS_LIBROSA are false, use_w2v2 is off): torch.stft(n_fft=400,
hop_length=160) magnitudes -> [mean, std, max, min] tiled and normalised; the 3-bin pooling into 64 bands; the energy proxy.

The clips: seeded 0.1 * randn at every length of LENGTHS (the edges of torch.stft's frame count and of its reflect padding), a sine,
an all-zero clip and a stereo clip.  Samples are rounded to the float16 grid before anything runs (they are stored as float16 and
are exact in float32), which halves the file.  Per clip: the wave, extract() at dim 128 and 6, the four float32 statistics (the
values of _torch_stft_fallback before tiling, recomputed the same way), generate(flatten=False), score(); the full magnitudes for
the clips of at most 561 samples only.  Data only.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SEED = 2027
LENGTHS = (201, 399, 400, 401, 559, 560, 561, 10079, 10080, 10240, 10241, 16000)
FULL_MAGNITUDE_UP_TO = 561


def clips(rng):
    """name -> (T,) or (C, T) float32 on the float16 grid."""
    c = {f"randn{n}": 0.1 * rng.standard_normal(n) for n in LENGTHS}
    t = np.arange(4000) / 16000.0
    c["sine4000"] = 0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * np.sin(2 * np.pi * 3100.0 * t + 0.3)
    c["zero1000"] = np.zeros(1000)
    c["stereo801"] = 0.1 * rng.standard_normal((2, 801))
    return {k: v.astype(np.float16).astype(np.float32) for k, v in c.items()}


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "src" / "core_blocks" / "audio_blocks.py").is_file():
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.modules["transformers"] = None
    sys.modules["librosa"] = None
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ref))
    import torch
    import src.core_blocks.audio_blocks as ab
    assert not ab._HAS_W2V2 and not ab._HAS_LIBROSA
    sf128, sf6 = ab.SpectralForensics(dim=128), ab.SpectralForensics(dim=6)
    assert not sf128.use_w2v2 and not sf6.use_w2v2
    mel, clone = ab.MelSpectrogramGenerator(), ab.VoiceCloneDetector()

    store = {"names": []}
    for name, wave in clips(np.random.default_rng(SEED)).items():
        mono, _ = ab._ensure_mono_16k(wave, 16000)
        spec = torch.stft(torch.from_numpy(mono).float(), n_fft=400, hop_length=160, return_complex=True).abs().numpy()
        stats = np.array([spec.mean(), spec.std(), spec.max(), spec.min()], dtype=np.float32)      # as _torch_stft_fallback builds them
        f128, f6 = sf128.extract(wave), sf6.extract(wave)
        assert np.array_equal(f128, sf128._torch_stft_fallback(mono)) and f128.shape == (128,) and f6.shape == (6,)
        n = np.linalg.norm(np.tile(stats, 32)) + 1e-9
        assert np.array_equal(f128, (np.tile(stats, 32) / n).astype(np.float32))
        m = mel.generate(wave, flatten=False)
        assert m.shape == (64, spec.shape[1]) and m.dtype == np.float32 and spec.shape == (201, 1 + mono.shape[0] // 160)
        store["names"].append(name)
        for key, val in (("wave", wave.astype(np.float16)), ("stats", stats), ("features128", f128), ("features6", f6), ("mel_like", m),
                         ("clone", np.float64(clone.score(wave)))):
            store[f"{name}/{key}"] = val
        if mono.shape[0] <= FULL_MAGNITUDE_UP_TO:
            store[f"{name}/magnitude"] = spec
        print(name, wave.shape, "frames", spec.shape[1], "stats", stats, "clone", store[f"{name}/clone"], flush=True)
    assert not store["zero1000/features128"].any()
    store["names"] = np.array(store["names"])
    path = HERE / "spectral.npz"
    np.savez_compressed(path, **store)
    assert path.stat().st_size < 300_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
