#!/usr/bin/env python3
"""Cost of train-mode encoder dropout (GPU box): bench.py's --train-encoders step (BERT-base L = 128 + ViT-B/32, B = 32, both
encoders trained) timed at p = 0 and p = 0.1 at every encoder dropout site, in alternating blocks (A/B/A/B...) on ONE trainer --
the probabilities are plain encoder attributes, read by every training forward -- so that both settings see the same clocks and
the same weights' trajectory.  Prints one JSON line and a short table.
usage: encoder_dropout_cost.py [--batch 32] [--steps 20] [--warmup 5] [--blocks 4] [--p 0.1]"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

import bench
bench._import_torch()        # (bench.py loads torch in its ranks only; this process is one)
from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
from ultrafnd_git_amd.temporal import TemporalSyncNet
from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache


def set_p(tr, p: float) -> None:
    tr.text_encoder.hidden_dropout_prob = tr.text_encoder.attention_probs_dropout_prob = p
    tr.visual_encoder.attention_dropout = p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4, help="blocks per setting, alternating")
    ap.add_argument("--p", type=float, default=0.1)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = args.batch
    torch.manual_seed(42)
    tenc, venc = BertTextEncoder().to(dev), ClipVisualEncoder().to(dev)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir="/tmp/ufnd_dropout_cost", batch_size=B, device=str(dev), use_graph=True,
                      encode_inline=True, seed=42, train_encoders=True)
    tsync = TemporalSyncNet(in_dim=768, out_dim=256).to(dev)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(64, seed=1), text_encoder=tenc, visual_encoder=venc, temporal_net=tsync)
    tr.fusion.train(); tr.clf.train()
    batches = bench.make_batches(B, 4, 42 + 2, dev)
    for p in (0.0, args.p):
        set_p(tr, p)
        for i in range(args.warmup):
            tr.train_step(batches[i % 4])
    ms = {0.0: [], args.p: []}
    for blk in range(2 * args.blocks):
        p = 0.0 if blk % 2 == 0 else args.p
        set_p(tr, p)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(args.steps):
            tr.train_step(batches[i % 4])
        torch.cuda.synchronize(dev)
        ms[p].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {p: sorted(v)[len(v) // 2] for p, v in ms.items()}
    print(json.dumps({"what": "train step with both encoders trained, ms per step at encoder dropout p = 0 and p", "p": args.p, "batch": B,
                      "steps_per_block": args.steps, "ms_per_step_p0": [round(x, 4) for x in ms[0.0]],
                      "ms_per_step_p": [round(x, 4) for x in ms[args.p]], "median_p0": round(med[0.0], 4), "median_p": round(med[args.p], 4),
                      "slowdown": round(med[args.p] / med[0.0] - 1.0, 4), "final_loss": float(tr.optim.state.read().loss)}))
    print(f"p = 0    : {med[0.0]:.3f} ms/step  (blocks {', '.join(f'{x:.3f}' for x in ms[0.0])})")
    print(f"p = {args.p:<5}: {med[args.p]:.3f} ms/step  (blocks {', '.join(f'{x:.3f}' for x in ms[args.p])})")
    print(f"slowdown : {100 * (med[args.p] / med[0.0] - 1):+.2f} %")


if __name__ == "__main__":
    main()
