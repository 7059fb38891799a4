#!/usr/bin/env python3
"""Cost of gradient accumulation (GPU box): bench.py's --train-encoders step (BERT-base L = 128 + ViT-B/32 at full depth, one frame,
B = 32 rows per micro-batch, both encoders trained) timed at grad_accum_steps k = 1 and k = 4 in alternating blocks (A/B/A/B...) on
ONE trainer -- the group size is a host attribute of the optimizer, switched between blocks with nothing pending -- so that both
settings see the same clocks and the same weights' trajectory.  Device events around every block, a warm-up of every shape first.
Reported: ms per MICRO-batch at each k (k = 4 saves three of four clip + AdamW + operand-refresh passes and pays three accumulate
passes and one fold), and the accumulate kernel's own time and achieved bytes / s over the joint arena (12 B per parameter, 8 B for
the group's first micro-batch, which copies).  Prints one JSON line and a short table.
usage: grad_accum_cost.py [--batch 32] [--opt-steps 20] [--warmup 3] [--blocks 3] [--k 4]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

import bench
bench._import_torch()        # (bench.py loads torch in its ranks only; this process is one)
from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
from ultrafnd_git_amd.temporal import TemporalSyncNet
from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache


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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--opt-steps", type=int, default=20, help="optimizer steps per block (k micro-batches each)")
    ap.add_argument("--warmup", type=int, default=3, help="optimizer steps per setting before anything is timed")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per setting, alternating")
    ap.add_argument("--k", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, K = args.batch, args.k
    torch.manual_seed(42)
    tenc, venc = BertTextEncoder().to(dev), ClipVisualEncoder().to(dev)
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir="/tmp/ufnd_grad_accum_cost", batch_size=B, device=str(dev), use_graph=True,
                      encode_inline=True, seed=42, train_encoders=True, grad_accum_steps=K)
    tsync = TemporalSyncNet(in_dim=768, out_dim=256).to(dev)
    tr = ForensicTrainer(cfg, cache=synthetic_cache(64, seed=1), text_encoder=tenc, visual_encoder=venc, temporal_net=tsync)
    tr.fusion.train(); tr.clf.train()
    batches = bench.make_batches(B, 4, 42 + 2, dev)
    o = tr.optim

    def set_k(k: int) -> None:
        assert o.pending == 0
        o.accum_steps = k
        tr.reducer.hold, tr.reducer.before_bucket = False, None

    for k in (1, K):
        set_k(k)
        for i in range(args.warmup * k):
            tr.train_step(batches[i % 4])
    ms = {1: [], K: []}
    for blk in range(2 * args.blocks):
        k = 1 if blk % 2 == 0 else K
        set_k(k)
        n = args.opt_steps * k
        ms[k].append(timed_ms(lambda i: tr.train_step(batches[i % 4]), n, dev))
        assert o.pending == 0 and int(o.state.read().micro) == 0
    set_k(K)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    # the accumulate pass alone over the joint arena (no state: the count is not part of the cost)
    a = tr.arena
    n = a.n_grad
    acc_ms = {}
    for name, overwrite in (("copy", True), ("add", False)):
        a.grad_acc.zero_()
        timed_ms(lambda i: o._accumulate(a.grad_acc, a.grad, 0, n, overwrite, None), 5, dev)
        acc_ms[name] = min(timed_ms(lambda i: o._accumulate(a.grad_acc, a.grad, 0, n, overwrite, None), 20, dev) for _ in range(3))
    gbs = {"copy": 8 * n / acc_ms["copy"] / 1e6, "add": 12 * n / acc_ms["add"] / 1e6}
    per_group = acc_ms["copy"] + (K - 2) * acc_ms["add"] + acc_ms["add"]        # k - 1 accumulates (the first copies) + one fold
    res = {"what": "train step with both encoders trained, ms per micro-batch at grad_accum_steps 1 and k", "k": K, "batch": B,
           "opt_steps_per_block": args.opt_steps, "arena_params": n,
           "ms_per_micro_batch_k1": [round(x, 4) for x in ms[1]], "ms_per_micro_batch_k": [round(x, 4) for x in ms[K]],
           "median_k1": round(med[1], 4), "median_k": round(med[K], 4), "change": round(med[K] / med[1] - 1.0, 4),
           "accumulate_ms": {k: round(v, 4) for k, v in acc_ms.items()}, "accumulate_GBps": {k: round(v, 1) for k, v in gbs.items()},
           "accumulate_ms_per_group": round(per_group, 4), "accumulate_share_of_a_micro_batch": round(per_group / K / med[K], 4),
           "final_loss": float(o.state.read().loss)}
    print(json.dumps(res))
    print(f"arena    : {n / 1e6:.1f} M trainable fp32 parameters")
    print(f"k = 1    : {med[1]:.3f} ms / micro-batch  (blocks {', '.join(f'{x:.3f}' for x in ms[1])})")
    print(f"k = {K:<5}: {med[K]:.3f} ms / micro-batch  (blocks {', '.join(f'{x:.3f}' for x in ms[K])})")
    print(f"change   : {100 * (med[K] / med[1] - 1):+.2f} % per micro-batch")
    print(f"accumulate: copy {acc_ms['copy']:.3f} ms ({gbs['copy']:.0f} GB/s at 8 B/param), add {acc_ms['add']:.3f} ms ({gbs['add']:.0f} GB/s at 12 B/param)")
    print(f"            {per_group:.3f} ms per group of {K} = {100 * per_group / K / med[K]:.2f} % of a micro-batch")


if __name__ == "__main__":
    main()
