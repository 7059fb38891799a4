"""Child of tests/test_gpu_grad_accum_dp.py, run under `python -m torch.distributed.run` (beside tests/dp_child.py, whose helpers it uses).

  --mode force1   world 1, backend nccl (= RCCL), grad_accum_steps = 2: ForensicTrainer(force_exchange=True) against the same steps
                  without an exchange -- a one-rank sum is the identity, so no bit may change -- and the number of bucket
                  reductions: one per bucket per OPTIMIZER step.
  --mode world2   two ranks sharing cuda:0 over gloo (host-staged, tests/host_staged.py -- not a product path): 2 ranks x 2
                  micro-batches x 8 rows against the single-process step over the same 32 rows.
Prints one JSON line on rank 0."""
import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch
import torch.distributed as dist

from dp_child import DEV, dict_batches, make_trainer


def _rows(b, lo, hi):
    return {k: v[lo:hi].contiguous() for k, v in b.items()}


def force1(out_dir):
    from ultrafnd_git_amd.dp import init_process_group
    init_process_group(DEV)
    B, K, STEPS = 8, 2, 2
    runs, res = {}, {}
    for tag, active in (("exchange", True), ("plain", False)):
        for graph in (True, False):
            torch.manual_seed(5)
            tr = make_trainer(out_dir, B, use_graph=graph, force_exchange=active, grad_accum_steps=K)
            assert tr.reducer.force == active and len(tr.reducer.buckets) == 2
            calls = []
            orig = tr.reducer._reduce
            tr.reducer._reduce = lambda lo, hi, _o=orig, _c=calls: (_c.append((lo, hi)), _o(lo, hi))[1]
            tr.fusion.train(); tr.clf.train()            # (dropout on: the micro-batch keys are part of what must not change)
            held = []
            for i, b in enumerate(dict_batches(B, K * STEPS, 11)):
                out = tr.train_step(b)
                held.append(bool(tr.reducer.hold))
            torch.cuda.synchronize()
            st = tr.optim.state.read()
            runs[(tag, graph)] = (tr.arena.data.clone(), out["logits"].clone(), float(st.grad_norm), int(st.step), int(st.micro))
            if active:
                res[f"reduce_calls_graph{int(graph)}"] = calls
                res[f"held_graph{int(graph)}"] = held
                res["buckets"] = [list(x) for x in tr.reducer.buckets]
    ref = runs[("plain", False)]
    res["bit_identical"] = all(torch.equal(v[0], ref[0]) and torch.equal(v[1], ref[1]) and v[2] == ref[2] for v in runs.values())
    res["steps"], res["micro"] = ref[3], ref[4]
    res["backend"] = dist.get_backend()
    print(json.dumps(res))
    dist.destroy_process_group()


def world2(out_dir):
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    B, K = 32, 2                                     # global rows per optimizer step; every rank takes K micro-batches of B / world / K
    batches = dict_batches(B, 3, 17)
    ref = None
    if rank == 0:                                    # single-process step over the 32 rows, BEFORE the group exists
        torch.manual_seed(5)
        tr0 = make_trainer(os.path.join(out_dir, "ref"), B, use_graph=False)
        tr0.fusion.dropout = tr0.clf.dropout = tr0.clf.node_dropout = 0.0
        tr0.head.step_bufs.clear()
        tr0.fusion.train(); tr0.clf.train()
        for b in batches:
            tr0.train_step(b)
        ref = (tr0.arena.data.clone(), float(tr0.optim.state.read().grad_norm))
        del tr0
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from host_staged import HostStagedCollectives
    comm = HostStagedCollectives()
    torch.manual_seed(5)
    mb = B // world // K
    tr = make_trainer(out_dir, mb, use_graph=True, group=comm, grad_accum_steps=K)
    assert tr.world == world and abs(tr.reducer.grad_scale - 0.5) < 1e-12
    tr.fusion.dropout = tr.clf.dropout = tr.clf.node_dropout = 0.0
    tr.head.step_bufs.clear()
    tr.fusion.train(); tr.clf.train()
    staged = []
    for b in batches:
        shard = {k: v[rank::world].contiguous() for k, v in b.items()}
        for j in range(K):
            before = comm.staged_calls
            tr.train_step(_rows(shard, mb * j, mb * j + mb))
            staged.append(comm.staged_calls - before)
    torch.cuda.synchronize()
    st = tr.optim.state.read()
    res = {"staged_per_micro_batch": staged, "steps": int(st.step), "grad_scale": float(st.grad_scale)}
    if rank == 0:
        res.update({"param_max_abs_err": (tr.arena.data - ref[0]).abs().max().item(), "param_scale": ref[0].abs().max().item(),
                    "grad_norm": float(st.grad_norm), "grad_norm_ref": ref[1]})
    mine = tr.arena.data.cpu()
    other = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(other, mine)
    res["ranks_agree"] = bool(all(torch.equal(o, other[0]) for o in other))
    if rank == 0:
        print(json.dumps(res))
    dist.destroy_process_group()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    {"force1": force1, "world2": world2}[a.mode](a.out)
