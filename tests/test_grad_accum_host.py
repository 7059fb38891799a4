"""CPU: the host side of gradient accumulation -- the TrainConfig option, the CLI flag and the step state's `micro` field."""
import ctypes
import dataclasses
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def _cfg(**kw):
    from ultrafnd_git_amd.trainer import TrainConfig
    return TrainConfig(data_root="", ocr_phrase_pkl=None, **kw)


def test_grad_accum_steps_is_an_init_only_option_not_a_field():
    from ultrafnd_git_amd.trainer import TrainConfig
    assert "grad_accum_steps" not in [f.name for f in dataclasses.fields(TrainConfig)]
    assert _cfg().grad_accum_steps == 1
    c = _cfg(grad_accum_steps=4)
    assert c.grad_accum_steps == 4 and type(c.grad_accum_steps) is int
    assert _cfg(grad_accum_steps=4, encoder_dropout=0.1).encoder_dropout == pytest.approx(0.1)


@pytest.mark.parametrize("bad", [0, -1, 2.5])
def test_grad_accum_steps_must_be_a_positive_integer(bad):
    with pytest.raises(ValueError, match="grad_accum_steps"):
        _cfg(grad_accum_steps=bad)


def test_factor_exchange_refuses_accumulation(tmp_path):
    """grad_exchange="factors" with k = 2 raises when the trainer is built, before anything touches a device; k = 1 gets past it."""
    from ultrafnd_git_amd import _lib as L
    from ultrafnd_git_amd.trainer import ForensicTrainer, synthetic_cache
    with pytest.raises(ValueError, match="factors.*grad_accum_steps=2"):
        ForensicTrainer(_cfg(out_dir=str(tmp_path), batch_size=8, grad_exchange="factors", grad_accum_steps=2, device="cpu"),
                        cache=synthetic_cache(16, seed=1))
    with pytest.raises(L.UltrafndHipError):          # (the next check: no CPU path)
        ForensicTrainer(_cfg(out_dir=str(tmp_path), batch_size=8, grad_exchange="factors", device="cpu"), cache=synthetic_cache(16, seed=1))


def test_cli_flag_parses_with_default_one(monkeypatch):
    sys.path.insert(0, str(REPO))
    import run_train_eval as R
    monkeypatch.setattr(sys, "argv", ["run_train_eval.py"])
    assert R.parse_args().grad_accum_steps == 1
    monkeypatch.setattr(sys, "argv", ["run_train_eval.py", "--grad_accum_steps", "4"])
    assert R.parse_args().grad_accum_steps == 4


def test_step_state_keeps_its_size_and_micro_takes_the_first_reserved_word():
    from ultrafnd_git_amd import _lib as L
    assert ctypes.sizeof(L.StepState) == 80 and L.ABI_VERSION == 6
    assert L.StepState.micro.offset == 64 == L.StepState.bc2_sqrt.offset + 4      # the old reserved[0]: two u64 + twelve floats in
    assert L.StepState.micro.size == 4 and L.StepState.reserved.offset == 68 and L.StepState.reserved.size == 8
    st = L.StepState()
    assert st.micro == 0


def test_reducer_hold_and_before_bucket():
    """GradReducer: `hold` makes the exchange inactive; start(k) calls before_bucket(lo, hi) in front of each bucket's reduction."""
    import torch
    from ultrafnd_git_amd.dp import Collectives, GradReducer

    class Two(Collectives):
        def __init__(self):
            self.group, self.world, self.rank, self.initialized = None, 2, 0, True
            self.log = []

        def all_reduce_async(self, t):
            self.log.append(("reduce", t.numel()))
            t.mul_(2.0)
            return None

    g = torch.ones(96)
    comm = Two()
    r = GradReducer(g, group=comm, bounds=[32])
    assert r.active and r.hold is False and r.before_bucket is None
    r.hold = True
    assert not r.active
    r.start()
    assert comm.log == []
    r.hold = False
    r.before_bucket = lambda lo, hi: (comm.log.append(("fold", lo, hi)), g[lo:hi].add_(1.0))
    r.start(1)
    r.start(0)
    r.finish()
    assert comm.log == [("fold", 32, 96), ("reduce", 64), ("fold", 0, 32), ("reduce", 32)]
    assert torch.equal(g, torch.full((96,), 4.0))
