#!/usr/bin/env python3
"""Cost of the raw-data recipe on the head-only step (GPU box): cached features, one train step = gather + the head's captured forward /
criterion / backward + clip + AdamW, at B = 32 and B = 256 for four configurations of ONE synthetic cache:

    ce_fused      plain CE, fused_head=True   (the default path: two C-ABI calls)
    ce_five_call  plain CE, fused_head=False  (five module-level calls, ufnd_softmax_ce)
    focal         criterion="focal"           (five calls, ufnd_softmax_focal in place of ufnd_softmax_ce)
    focal_mixup   criterion="focal", mixup_alpha=0.2, mixup_prob=1.0 (ufnd_gather_mix_rows in place of ufnd_gather_rows, one small
                  host-to-device copy of the draw per step)

timed in alternating blocks (A/B/C/D/A/B/C/D...) so that all four see the same clocks, device events around every block, every
configuration warmed up first (its graph captured).  Reported: the median block's ms per step, and focal_mixup over ce_five_call --
the same five-call path with the two new kernels.  Writes --out when given.
usage: focal_mixup_cost.py [--steps 200] [--warmup 20] [--blocks 5] [--out profiles/focal_mixup_cost.txt]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache

CONFIGS = {"ce_fused": dict(fused_head=True), "ce_five_call": dict(fused_head=False), "focal": dict(criterion="focal"),
           "focal_mixup": dict(criterion="focal", mixup_alpha=0.2, mixup_prob=1.0)}


def timed_ms(fn, n: int, dev) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="train steps per block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5, help="blocks per configuration, alternating")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    prop = torch.cuda.get_device_properties(0)
    lines = [f"head-only train step on cached features, ms per step ({prop.name}, {getattr(prop, 'gcnArchName', '?')}; device events around blocks of "
             f"{args.steps} steps, {args.blocks} blocks per configuration in alternation, median block; hipGraph replay)", ""]
    res = {}
    for B in (32, 256):
        cache = synthetic_cache(4 * B + 64, seed=1)
        runs = {}
        for name, kw in CONFIGS.items():
            torch.manual_seed(42)
            cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir="/tmp/ufnd_focal_mixup_cost", batch_size=B, device=str(dev), use_graph=True,
                              seed=42, **kw)
            tr = ForensicTrainer(cfg, cache=cache)
            tr.fusion.train(); tr.clf.train()
            batches = [b for b in tr.train_loader if b["index"].numel() == B][:4]
            assert len(batches) >= 2 and tr.head.fused_entries == (name == "ce_fused")
            step = lambda i, tr=tr, batches=batches: tr.train_step(batches[i % len(batches)])
            for i in range(args.warmup):
                step(i)
            runs[name] = step
        ms = {name: [] for name in CONFIGS}
        for _ in range(args.blocks):
            for name, step in runs.items():
                ms[name].append(timed_ms(step, args.steps, dev))
        med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
        res[B] = {"median_ms": {k: round(v, 4) for k, v in med.items()}, "blocks_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                  "focal_mixup_over_ce_five_call": round(med["focal_mixup"] / med["ce_five_call"], 4),
                  "focal_over_ce_five_call": round(med["focal"] / med["ce_five_call"], 4),
                  "ce_five_call_over_ce_fused": round(med["ce_five_call"] / med["ce_fused"], 4)}
        lines.append(f"B = {B}")
        for name in CONFIGS:
            lines.append(f"  {name:14s} {med[name]:8.4f} ms   (blocks {', '.join(f'{x:.4f}' for x in ms[name])})")
        lines += [f"  focal_mixup / ce_five_call = {res[B]['focal_mixup_over_ce_five_call']:.4f}   focal / ce_five_call = {res[B]['focal_over_ce_five_call']:.4f}"
                  f"   ce_five_call / ce_fused = {res[B]['ce_five_call_over_ce_fused']:.4f}", ""]
    print(json.dumps(res))
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
