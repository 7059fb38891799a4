#!/usr/bin/env python3
"""Throughput of the CLIP text tower (ultrafnd_git_amd/semantic.py: ClipTextEncoder, 12 layers) on one MI355X: one process, one GPU,
unprofiled.

    clip_text_throughput.py [--out profiles/clip_text_throughput.txt]
        titles/s at B = 32 and B = 256, for token counts drawn uniformly from 8..40 (padded to 77, CLIP's tokenizer habit) and for
        all-77: the packed (live-row) pass against the padded one; causal skipping on against off; the 2-wave, 64-query attention form
        against the 4-wave, 128-query one; and, on the same device and weights, HF's CLIPTextModelWithProjection in bf16, batched.
    clip_text_throughput.py --build
        only builds the two experiment libraries (no GPU needed): libultrafnd_hip_noskip.so (-DUFND_CAUSAL_SKIP=0) and
        libultrafnd_hip_wide.so (-DUFND_CAUSAL_WAVES=4), beside the product library, with the product's own build recipe.

Device events around windows of >= 0.5 s after warm-up, three windows per path, the paths alternated; median.  The experiment builds
are loaded into the same process and swapped in under the encoder between windows, so every path sees the same weights, buffers and
clocks.  Run it under a `timeout`.
"""
import argparse
import ctypes
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ultrafnd_git_amd import build as Bd

VARIANTS = {"noskip": ["UFND_CAUSAL_SKIP=0"], "wide": ["UFND_CAUSAL_WAVES=4"]}
L77, LAYERS = 77, 12


def variant_lib(name):
    """The experiment library `name`, built if its stamp is stale (a no-op after --build on the same tree)."""
    Bd.EXTRA_DEFS[:] = VARIANTS[name]
    try:
        return Bd._build_one(Bd.PKG / f"libultrafnd_hip_{name}.so", Bd.sources(), name, [], False, False)
    finally:
        Bd.EXTRA_DEFS[:] = []


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--build", action="store_true")
ap.add_argument("--window", type=float, default=0.5)
a = ap.parse_args()
paths = {n: variant_lib(n) for n in VARIANTS}
if a.build:
    print("\n".join(str(p) for p in paths.values()))
    sys.exit(0)

import torch

from ultrafnd_git_amd import _lib as L
from ultrafnd_git_amd.semantic import ClipTextEncoder

if not torch.cuda.is_available():
    raise SystemExit("clip_text_throughput.py: no HIP device (timings are taken on the GPU only)")
DEV = torch.device("cuda")
LIBS = {"product": L.lib()}
for n, p in paths.items():
    LIBS[n] = ctypes.CDLL(str(p))
    L._declare(LIBS[n])


def timed(fn, window_s):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(2, int(window_s / max(time.perf_counter() - t0, 1e-5)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def batch(B, dist, eos):
    """(B, 77) ids padded with EOS and the mask of ones up to the EOS: token counts (EOS included) uniform in 8..40, or all 77."""
    g = torch.Generator().manual_seed(B)
    n = torch.randint(8, 41, (B,), generator=g) if dist == "8..40" else torch.full((B,), L77)
    ids = torch.randint(3, eos - 1, (B, L77), generator=g)
    pos = torch.arange(L77)[None, :]
    ids[pos >= n[:, None] - 1] = eos
    return ids.to(DEV), (pos < n[:, None]).to(torch.int32).to(DEV), float(n.float().mean())


out = []


def say(s):
    print(s, flush=True)
    out.append(s)


enc = ClipTextEncoder(num_hidden_layers=LAYERS).to(DEV)
from transformers import CLIPTextConfig, CLIPTextModelWithProjection

hf = CLIPTextModelWithProjection(CLIPTextConfig(num_hidden_layers=LAYERS)).eval()
hf.load_state_dict(enc.state_dict(), strict=True)
hf = hf.to(DEV, torch.bfloat16)
prop = torch.cuda.get_device_properties(0)
say(f"# tools/clip_text_throughput.py on one {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}: ClipTextEncoder, {LAYERS} layers, "
    f"L = {L77}, seeded weights; device events over windows of >= {a.window} s after warm-up, three windows per path (alternated), median; "
    "ids and masks device-resident; unprofiled.")
say("# paths: packed / padded = the product library; noskip = built with -DUFND_CAUSAL_SKIP=0 (every key block walked, the diagonal test "
    "everywhere); wide = built with -DUFND_CAUSAL_WAVES=4 (the 4-wave, 128-query attention form); HF bf16 = CLIPTextModelWithProjection, "
    "batched, same device and weights (its default attention implementation)")


def native(lib, ids, mask, packed):
    def run():
        L._lib = LIBS[lib]
        try:
            return enc(ids, mask, packed=packed)
        finally:
            L._lib = LIBS["product"]
    return run


with torch.no_grad():
    for B in (32, 256):
        for dist in ("8..40", "all-77"):
            ids, mask, mean_n = batch(B, dist, enc.eos_token_id)
            mask64 = mask.long()

            def hf_bf16():
                return torch.nn.functional.normalize(hf(input_ids=ids, attention_mask=mask64).text_embeds.float(), dim=-1)

            legs = [("packed", native("product", ids, mask, True)), ("padded", native("product", ids, mask, False)),
                    ("packed noskip", native("noskip", ids, mask, True)), ("padded noskip", native("noskip", ids, mask, False)),
                    ("packed wide", native("wide", ids, mask, True)), ("padded wide", native("wide", ids, mask, False)), ("HF bf16", hf_bf16)]
            ref = legs[0][1]().clone()
            same = {nm: bool(torch.equal(fn(), ref)) for nm, fn in legs[:-1]}
            say(f"B={B} tokens {dist} (mean {mean_n:.1f} of {L77} rows live): features bit-identical to packed: "
                + ", ".join(f"{k}={v}" for k, v in same.items()) + f"; HF bf16 vs packed max-abs {float((hf_bf16() - ref).abs().max()):.2e}")
            res = {nm: [] for nm, _ in legs}
            for _ in range(3):
                for nm, fn in legs:
                    res[nm].append(timed(fn, a.window))
            for nm, _ in legs:
                ms = [m for m, _ in res[nm]]
                med = statistics.median(ms)
                say(f"  B={B} {dist:7s} {nm:14s} {med:7.3f} ms per call = {B / med * 1e3:9.0f} titles/s (three windows: "
                    f"{', '.join(f'{m:.3f}' for m in ms)}; {res[nm][0][1]} calls per window)")
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
