"""Child of tests/test_gpu_focal_mixup.py, run under `python -m torch.distributed.run` (beside tests/dp_child.py, whose helpers it uses).

World 1, backend nccl (= RCCL): ForensicTrainer(force_exchange=True) with the focal criterion and mixup, captured and eager, against the
same three steps without an exchange.  A one-rank sum is the identity and the draw does not depend on the exchange: no bit may change.
Prints one JSON line."""
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

from dp_child import DEV, make_trainer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    out_dir = ap.parse_args().out
    from ultrafnd_git_amd.dp import init_process_group
    init_process_group(DEV)
    B, STEPS = 16, 3
    runs = {}
    for active, graph in ((True, True), (True, False), (False, False)):
        torch.manual_seed(5)
        tr = make_trainer(out_dir, B, use_graph=graph, force_exchange=active, criterion="focal", mixup_alpha=0.2, mixup_prob=1.0,
                          mixup_mode="per_modality")
        assert tr.reducer.force == active and tr.reducer.active == active and not tr.head.fused_entries
        tr.fusion.train(); tr.clf.train()
        it = iter(tr.train_loader)
        for _ in range(STEPS):
            out = tr.train_step(next(it))
        torch.cuda.synchronize()
        st = tr.optim.state.read()
        runs[(active, graph)] = (tr.arena.data.clone(), out["logits"].clone(), float(st.grad_norm), float(st.loss), int(st.step))
    ref = runs[(False, False)]
    res = {"bit_identical": all(torch.equal(v[0], ref[0]) and torch.equal(v[1], ref[1]) and v[2:] == ref[2:] for v in runs.values()),
           "steps": ref[4], "loss": ref[3], "backend": dist.get_backend()}
    print(json.dumps(res))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
