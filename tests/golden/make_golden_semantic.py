#!/usr/bin/env python3
"""Mint tests/golden/semantic.npz from the REAL reference's SemanticForgeryAnalyzer (src/models/semantic_forgery.py).

Run in the build container only (needs /root/reference, which never travels):

    python tests/golden/make_golden_semantic.py

`transformers` is masked before the import (as make_golden.py does), so the reference takes its own "transformers is
optional" branch: no CLIP is constructed and no name-based from_pretrained loader is ever reached.  Its encode_text is replaced by
stored unit vectors (the l2n-ed CLIP features the head consumes), the module runs in eval mode (its Dropout(0.3) is the identity)
at proj_dim = 128 and B = 5, and the inputs, the four parameters and the three outputs are stored.  Data only.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
B, PROJ_DIM, SEED = 5, 128, 2024


def main():
    sys.modules["transformers"] = None
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    from src.models.semantic_forgery import SemanticConfig, SemanticForgeryAnalyzer

    torch.manual_seed(SEED)
    an = SemanticForgeryAnalyzer(SemanticConfig(proj_dim=PROJ_DIM), device=torch.device("cpu")).eval()
    assert not an.use_clip
    g = torch.Generator().manual_seed(SEED + 1)
    feats = {}
    for side in ("title", "ocr"):
        x = torch.randn(B, 512, generator=g)
        feats[side] = x / x.norm(dim=-1, keepdim=True)
    names = {side: [f"{side}{b}" for b in range(B)] for side in feats}
    table = {n: feats[side][b] for side in feats for b, n in enumerate(names[side])}
    an.encode_text = lambda texts: torch.stack([table[t] for t in texts])
    with torch.no_grad():
        out = an({"title": names["title"], "ocr": names["ocr"]})
    store = {"text_feat": feats["title"].numpy(), "image_feat": feats["ocr"].numpy()}
    for k, v in an.state_dict().items():
        store["param/" + k] = v.numpy()
    for k, v in out.items():
        store["out/" + k] = v.numpy()
    assert sorted(k for k in store if k.startswith("param/")) == ["param/text_proj.0.bias", "param/text_proj.0.weight", "param/vision_proj.0.bias",
                                                                 "param/vision_proj.0.weight"]
    path = HERE / "semantic.npz"
    np.savez_compressed(path, **store)
    assert path.stat().st_size < 1_000_000, path.stat().st_size
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
