#!/usr/bin/env python3
"""Mint tests/golden/affective.npz from the REAL reference's AffectiveForensics (src/models/affective_forensics.py).

Needs a checkout of the reference project (it is not part of this repository and never travels with it):

    python tests/golden/make_golden_affective.py <path to the reference checkout>

`transformers` is masked before the import (as make_golden_semantic.py does), so the reference's optional-dependency import fails
after `torch` is bound in its module and no name-based from_pretrained loader can be reached.  On the constructed object the text
branch is then switched on by hand: use_text_model = True, device = cpu, labels = id2label, `tok` a stub whose result has .to() and
carries the text as its key, `txt_model` a stub that returns stored float32 logits (1, 7) for that key.  analyze(text, audio) runs on
eight texts -- one empty, two with audio=None, clips of a few lengths -- and the logits, names, clips and every returned number are
stored.  This pins the reference's own post-processing (softmax, grouping, intensity / valence, the RMS-energy arousal: librosa is
absent, so the reference takes that branch itself); the encoder above it is third-party.  Data only.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
SEED = 2025
LABELS = ("anger", "disgust", "fear", "joy", "neutral", "sadness", "surprise")
CLIP_LENGTHS = (-1, 1, 63, 64, -1, 4097, 8000, 65)      # -1: audio=None
EMPTY = 2                                                  # the text that is ""


class _Encoded(dict):
    def to(self, device):
        return self


def main():
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / "src" / "models" / "affective_forensics.py").is_file():
        raise SystemExit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.modules["transformers"] = None
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(ref))
    import src.models.affective_forensics as ref_mod
    assert not ref_mod._HAS_TXT and not ref_mod._HAS_LIBROSA and ref_mod.torch is torch

    g = torch.Generator().manual_seed(SEED)
    N = len(CLIP_LENGTHS)
    logits = (2.5 * torch.randn(N, len(LABELS), generator=g)).float()
    texts = ["" if i == EMPTY else f"text{i}" for i in range(N)]
    table = {t: logits[i][None] for i, t in enumerate(texts) if t}
    af = ref_mod.AffectiveForensics()
    assert not af.use_text_model
    af.use_text_model, af.device, af.labels = True, torch.device("cpu"), dict(enumerate(LABELS))
    af.tok = lambda text, **kw: _Encoded(key=text)
    af.txt_model = lambda key: SimpleNamespace(logits=table[key])

    clips, out = [], {k: [] for k in ("probs", "intensity", "arousal", "valence")}
    for i, n in enumerate(CLIP_LENGTHS):
        audio = None if n < 0 else (0.4 * torch.randn(n, generator=g) * (0.3 + 0.2 * i)).numpy().astype(np.float32)
        clips.append(np.zeros(0, np.float32) if audio is None else audio)
        r = af.analyze(texts[i], audio)
        out["probs"].append([r["probs"]["fear"], r["probs"]["anger"], r["probs"]["joy"]])
        for k in ("intensity", "arousal", "valence"):
            out[k].append(r[k])
    store = {"logits": logits.numpy(), "labels": np.array(LABELS), "text_valid": np.array([1 if t else 0 for t in texts], np.int32),
             "clip_lengths": np.array(CLIP_LENGTHS, np.int32), "clips": np.concatenate(clips)}
    for k, v in out.items():
        store["out/" + k] = np.asarray(v, np.float64)
    assert store["out/probs"][EMPTY].tolist() == [0.0, 0.0, 0.0] and store["out/arousal"][0] == 0.5
    path = HERE / "affective.npz"
    np.savez_compressed(path, **store)
    assert path.stat().st_size < 1_000_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
