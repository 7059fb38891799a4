"""GPU: gradient accumulation under the data-parallel exchange, on the one MI355X this box has.  Like tests/test_gpu_dp.py, each test
runs a fresh process tree under `python -m torch.distributed.run` (started by tests/launcher.py): tests/grad_accum_dp_child.py does
the work and prints one JSON line.  At most two GPU processes at a time; the launcher ends a job at its time limit."""
import json
import socket
import sys

import pytest

pytestmark = pytest.mark.gpu


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(launch_job, nproc, mode, out_dir):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), "tests/grad_accum_dp_child.py", "--mode", mode, "--out", str(out_dir)]
    r = launch_job(cmd, env={"HSA_ENABLE_IPC_MODE_LEGACY": "0"}, timeout=300)
    assert r["rc"] == 0, (r["rc"], r["out"][-3000:], r["err"][-6000:])
    return json.loads([ln for ln in r["out"].splitlines() if ln.startswith("{")][-1])


def test_forced_rccl_exchange_with_accumulation_changes_no_bit_and_runs_once_per_optimizer_step(launch_job, tmp_path):
    """torchrun world 1, RCCL, force_exchange, k = 2, two optimizer steps (four micro-batches, dropout on), captured and eager: the
    arena, the last logits and the gradient norm are bit-identical to k = 2 without an exchange; every bucket was reduced once per
    optimizer step -- in gradient-ready order, on the group's last micro-batch -- and the first micro-batch of each group held the
    exchange back."""
    res = _run(launch_job, 1, "force1", tmp_path)
    assert res["backend"] == "nccl" and res["steps"] == 2 and res["micro"] == 0
    assert res["bit_identical"], res
    buckets = res["buckets"]
    assert len(buckets) == 2
    for g in (0, 1):
        assert res[f"reduce_calls_graph{g}"] == buckets * 2, res
        assert res[f"held_graph{g}"] == [True, False, True, False], res


def test_two_ranks_two_micro_batches_of_eight_equal_the_full_batch_step_of_32(launch_job, tmp_path):
    """Two ranks sharing the GPU (gloo, host-staged -- not a product path), each 2 micro-batches x 8 rows per optimizer step, three
    steps, against the single-process step over the same 32 rows, at test_two_ranks_on_one_gpu_equal_the_full_batch_step's
    tolerances; the ranks end bit-identical; only the last micro-batch of a group exchanged anything."""
    res = _run(launch_job, 2, "world2", tmp_path)
    assert res["ranks_agree"] and res["steps"] == 3 and res["grad_scale"] == 0.25, res
    assert res["param_max_abs_err"] <= 2e-5 * max(1.0, res["param_scale"]), res
    assert abs(res["grad_norm"] - res["grad_norm_ref"]) <= 1e-4 * max(1.0, res["grad_norm_ref"]), res
    staged = res["staged_per_micro_batch"]
    assert len(staged) == 6 and all(s == 0 for s in staged[0::2]) and all(s == 2 for s in staged[1::2]), res
