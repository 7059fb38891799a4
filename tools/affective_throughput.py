#!/usr/bin/env python3
"""Throughput of the RoBERTa emotion classifier (ultrafnd_git_amd/affective.py: RobertaEmotionClassifier, 6 layers, full vocabulary) on
one MI355X: one process, one GPU, unprofiled.

    affective_throughput.py [--out profiles/affective_throughput.txt]
        texts/s at B = 32 and B = 256, for token counts drawn uniformly from 8..40 (padded to 128) and for all-128, where nothing can
        be dropped: the packed (live-row) pass against the padded one, cls_tail on against off, AffectiveForensics.analyze_batch on
        top of the packed pass and, on the same device and weights, HF's RobertaForSequenceClassification in bf16, batched.

Device events around windows of >= 0.5 s after warm-up, three windows per path, the paths alternated; median.  Run it under a `timeout`.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch

from ultrafnd_git_amd.affective import AffectiveForensics, RobertaEmotionClassifier

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--window", type=float, default=0.5)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("affective_throughput.py: no HIP device (timings are taken on the GPU only)")
DEV = torch.device("cuda")
L128, LAYERS = 128, 6


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


def batch(B, dist, vocab, pad):
    """(B, 128) ids = <s> words </s> pad ... and the prefix mask: token counts uniform in 8..40, or all 128."""
    g = torch.Generator().manual_seed(B)
    n = torch.randint(8, 41, (B,), generator=g) if dist == "8..40" else torch.full((B,), L128)
    ids = torch.randint(3, vocab, (B, L128), generator=g)
    pos = torch.arange(L128)[None, :]
    ids[:, 0] = 0
    ids[pos == n[:, None] - 1] = 2
    ids[pos >= n[:, None]] = pad
    return ids.to(DEV), (pos < n[:, None]).to(torch.int32).to(DEV), float(n.float().mean())


out = []


def say(s):
    print(s, flush=True)
    out.append(s)


enc = RobertaEmotionClassifier(num_hidden_layers=LAYERS).to(DEV)
af = AffectiveForensics(classifier=enc, device=DEV)
from transformers import RobertaConfig, RobertaForSequenceClassification

cfg = RobertaConfig(vocab_size=enc.vocab, num_hidden_layers=LAYERS, hidden_size=enc.hidden, num_attention_heads=enc.heads, intermediate_size=enc.inter,
                    max_position_embeddings=enc.max_position, type_vocab_size=1, layer_norm_eps=enc.eps, pad_token_id=enc.pad_token_id,
                    num_labels=enc.num_labels)
hf = RobertaForSequenceClassification(cfg).eval()
hf.load_state_dict(enc.state_dict(), strict=True)
hf = hf.to(DEV, torch.bfloat16)
prop = torch.cuda.get_device_properties(0)
say(f"# tools/affective_throughput.py on one {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}: RobertaEmotionClassifier, "
    f"{LAYERS} layers, vocabulary {enc.vocab}, L = {L128}, seeded weights; device events over windows of >= {a.window} s after warm-up, three "
    "windows per path (alternated), median; ids and masks device-resident; unprofiled.")
say("# paths: packed / padded x cls_tail on / off = RobertaEmotionClassifier.logits; analyze = AffectiveForensics.analyze_batch (packed, cls_tail on, "
    "no audio); HF bf16 = RobertaForSequenceClassification, batched, same device and weights (its default attention implementation)")


def native(ids, mask, packed, tail):
    def run():
        enc.cls_tail = tail
        return enc.logits(ids, mask, packed=packed)
    return run


slower = []
with torch.no_grad():
    for B in (32, 256):
        for dist in ("8..40", "all-128"):
            ids, mask, mean_n = batch(B, dist, enc.vocab, enc.pad_token_id)
            mask64 = mask.long()

            def hf_bf16():
                return hf(input_ids=ids, attention_mask=mask64).logits.float()

            def analyze():
                enc.cls_tail = True
                return af.analyze_batch(ids, mask)["intensity"]

            legs = [("packed tail", native(ids, mask, True, True)), ("packed all-rows", native(ids, mask, True, False)),
                    ("padded tail", native(ids, mask, False, True)), ("padded all-rows", native(ids, mask, False, False)), ("analyze", analyze),
                    ("HF bf16", hf_bf16)]
            ref = legs[0][1]().clone()
            same = {nm: bool(torch.equal(fn(), ref)) for nm, fn in legs[1:4]}
            say(f"B={B} tokens {dist} (mean {mean_n:.1f} of {L128} rows live): logits bit-identical to packed tail: "
                + ", ".join(f"{k}={v}" for k, v in same.items()) + f"; HF bf16 vs packed max-abs {float((hf_bf16() - ref).abs().max()):.2e}")
            res = {nm: [] for nm, _ in legs}
            for _ in range(3):
                for nm, fn in legs:
                    res[nm].append(timed(fn, a.window))
            med = {}
            for nm, _ in legs:
                ms = [m for m, _ in res[nm]]
                med[nm] = statistics.median(ms)
                say(f"  B={B} {dist:7s} {nm:16s} {med[nm]:7.3f} ms per call = {B / med[nm] * 1e3:9.0f} texts/s (three windows: "
                    f"{', '.join(f'{m:.3f}' for m in ms)}; {res[nm][0][1]} calls per window)")
            if med["packed tail"] > med["packed all-rows"]:
                slower.append(f"B={B} {dist}")
say("# cls_tail (packed pass) slower than the all-rows pass at: " + (", ".join(slower) if slower else "no batch"))
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(out) + "\n")
