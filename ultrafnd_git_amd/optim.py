"""clip_grad_norm_ + AdamW + StepLR over the flat arena (forensic_trainer.py:173-177,292-298,341).

Two streaming kernels replace the reference's ~104 per-tensor norms and its foreach AdamW:
`ufnd_grad_norm` (4 B/param) and `ufnd_adamw_step` (28 B/param), both over the arena's
contiguous with-grad range.  Hyper-parameters live in the device step state so a captured
graph sees lr changes.

Gradient accumulation (`accum_steps = k > 1`): one optimizer step per k micro-batches.  Every backward still overwrites
`arena.grad`; after a micro-batch that is not the group's last, `accumulate()` moves it into `arena.grad_acc`
(`ufnd_grad_accumulate`: copy for the first, add for the others) and counts the micro-batch in the step state, which re-keys the
dropout masks.  After the last one the accumulator is added back into `arena.grad` (`fold`, whole or bucket by bucket in front
of the gradient exchange), so norm, clip, AdamW and `.grad` see the group's SUM, and `grad_scale` carries the 1 / k' of the
mean over the k' micro-batches of the group (k' < k for a group cut short: `load_acc` + step).
"""
from __future__ import annotations

import math
from typing import List

import torch

from . import _lib as L
from .arena import FlatArena
from .state import StepStateBuffer


class FusedAdamW:
    def __init__(self, arena: FlatArena, lr: float = 2e-4, weight_decay: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, max_norm: float = 5.0, seed: int = 0, grad_scale: float = 1.0, accum_steps: int = 1):
        if arena.device.type != "cuda":
            raise L.UltrafndHipError("FusedAdamW needs the parameter arena on a HIP device (no CPU fallback)")
        self.arena = arena
        self.state = StepStateBuffer(arena.device, seed=seed, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps,
                                     max_norm=max_norm if max_norm else 0.0, grad_scale=grad_scale)
        self.param_groups: List[dict] = [{"lr": lr, "initial_lr": lr, "weight_decay": weight_decay, "betas": betas,
                                          "eps": eps}]
        self._partials = torch.empty(1024, dtype=torch.float32, device=arena.device)
        self.fused = True          # ufnd_clip_adamw_step (two launches) instead of norm + finalize + AdamW + advance (four)
        arena.ensure_grad()
        arena.ensure_moments()
        if isinstance(accum_steps, bool) or int(accum_steps) != accum_steps or int(accum_steps) < 1:
            raise ValueError(f"accum_steps={accum_steps!r}: an integer >= 1 (micro-batches per optimizer step)")
        self.accum_steps = int(accum_steps)
        self.pending = 0                       # micro-batches in the accumulator (host count; the device's is state.micro)
        self._base_scale = float(grad_scale)   # the exchange's 1 / world
        self._group = 1                        # the k' that state.grad_scale = _base_scale / k' currently holds
        if self.accum_steps > 1:
            arena.ensure_grad_acc()

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Kept for API parity (forensic_trainer.py:290).  Gradients are overwritten by every backward and the accumulator
        by the first micro-batch of every group (`accumulate`), so there is nothing to clear."""

    def set_lr(self, lr: float) -> None:
        self.param_groups[0]["lr"] = lr
        self.state.set_float("lr", lr)

    # ---- gradient accumulation (module docstring)
    def _accumulate(self, dst: torch.Tensor, src: torch.Tensor, lo: int, hi: int, overwrite: bool, state) -> None:
        if not (0 <= lo < hi <= self.arena.n_grad):
            raise ValueError(f"gradient range [{lo}, {hi}) outside the arena's [0, {self.arena.n_grad})")
        L.check(L.lib().ufnd_grad_accumulate(dst.data_ptr() + 4 * lo, src.data_ptr() + 4 * lo, hi - lo, int(overwrite), state,
                                             L.stream_ptr(self.arena.device)), "ufnd_grad_accumulate")

    def _acc(self) -> torch.Tensor:
        if self.arena.grad_acc is None:
            raise L.UltrafndHipError("no gradient accumulator: construct FusedAdamW with accum_steps > 1")
        return self.arena.grad_acc

    def accumulate(self) -> None:
        """After the backward of a micro-batch that is not its group's last: acc (= | +=) grad, and state.micro += 1.  Enqueue it
        on the step's main stream with every side stream of the backward joined: the launch re-keys the dropout masks, and the
        backward it follows regenerates the masks of the forward it belongs to."""
        a = self.arena
        self._accumulate(self._acc(), a.grad, 0, a.n_grad, self.pending == 0, self.state.ptr)
        self.pending += 1

    def fold(self, lo: int, hi: int) -> None:
        """grad[lo:hi] += acc[lo:hi]: the last micro-batch's gradients become the group's sum (no state: it is not counted)."""
        self._accumulate(self.arena.grad, self._acc(), int(lo), int(hi), False, None)

    def load_acc(self) -> None:
        """grad = acc: the pending micro-batches alone (a group cut short)."""
        a = self.arena
        self._accumulate(a.grad, self._acc(), 0, a.n_grad, True, None)

    def set_group(self, micro_batches: int) -> None:
        """state.grad_scale = (1 / world) / k' for a group of k' micro-batches; written only when k' changes."""
        kp = int(micro_batches)
        if kp < 1:
            raise ValueError(f"a group of {kp} micro-batches")
        if kp != self._group:
            self.state.set_float("grad_scale", self._base_scale / kp)
            self._group = kp

    def clip_and_step(self) -> None:
        """nn.utils.clip_grad_norm_(params, max_norm) followed by optim.step()."""
        a, dev = self.arena, self.arena.device
        s = L.stream_ptr(dev)
        lib = L.lib()
        if self.fused:       # two launches: sum of squares (+ step counter), then norm / clip / AdamW
            L.check(lib.ufnd_clip_adamw_step(a.data.data_ptr(), a.grad.data_ptr(), a.exp_avg.data_ptr(), a.exp_avg_sq.data_ptr(), a.n_grad,
                                             self._partials.data_ptr(), self.state.ptr, s), "ufnd_clip_adamw_step")
            return
        L.check(lib.ufnd_grad_norm(a.grad.data_ptr(), a.n_grad, self._partials.data_ptr(), self.state.ptr, s),
                "ufnd_grad_norm")
        L.check(lib.ufnd_adamw_step(a.data.data_ptr(), a.grad.data_ptr(), a.exp_avg.data_ptr(),
                                    a.exp_avg_sq.data_ptr(), a.n_grad, self.state.ptr, s), "ufnd_adamw_step")
        L.check(lib.ufnd_step_advance(self.state.ptr, s), "ufnd_step_advance")

    step = clip_and_step

    def state_dict(self) -> dict:
        st = self.state.read()
        return {"step": int(st.step), "lr": float(st.lr), "exp_avg": self.arena.exp_avg.clone(),
                "exp_avg_sq": self.arena.exp_avg_sq.clone()}


class StepLR:
    """torch.optim.lr_scheduler.StepLR(optim, step_size, gamma) for FusedAdamW (forensic_trainer.py:177)."""

    def __init__(self, optimizer: FusedAdamW, step_size: int, gamma: float = 0.1):
        self.optimizer, self.step_size, self.gamma = optimizer, int(step_size), float(gamma)
        self.base_lr = optimizer.param_groups[0]["initial_lr"]
        self.last_epoch = 0

    def step(self) -> None:
        self.last_epoch += 1
        self.optimizer.set_lr(self.base_lr * self.gamma ** (self.last_epoch // self.step_size))

    def get_last_lr(self):
        return [self.optimizer.param_groups[0]["lr"]]


class CosineAnnealingLR:
    """torch.optim.lr_scheduler.CosineAnnealingLR(optim, T_max, eta_min) for FusedAdamW (closed form), the
    integrated variant's schedule (forensic_trainer_integrated.py:151-155: T_max = epochs, eta_min = lr * min_lr_scale)."""

    def __init__(self, optim: FusedAdamW, T_max: int, eta_min: float = 0.0):
        import math
        self._math = math
        self.optim, self.T_max, self.eta_min = optim, max(1, int(T_max)), float(eta_min)
        self.base_lr = optim.param_groups[0]["initial_lr"]
        self.last_epoch = 0

    def get_last_lr(self):
        return [self.optim.param_groups[0]["lr"]]

    def step(self) -> None:
        self.last_epoch += 1
        lr = self.eta_min + (self.base_lr - self.eta_min) * (1 + self._math.cos(self._math.pi * self.last_epoch / self.T_max)) / 2
        self.optim.set_lr(lr)


class CosineAnnealingWarmRestarts:
    """torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optim, T_0, T_mult, eta_min) for FusedAdamW (closed form), the raw-data
    trainer's schedule (run_train_eval.py:726,729: T_0 = 5 | 10, T_mult = 2, eta_min = 1e-6).  Stepped once per epoch; T_cur and
    T_i are kept as torch's class keeps them when step() is called without an argument, and the expression is torch's, operation
    by operation, so the learning rates agree to the last bit of the double."""

    def __init__(self, optim: FusedAdamW, T_0: int, T_mult: int = 1, eta_min: float = 0.0):
        if isinstance(T_0, bool) or not isinstance(T_0, int) or T_0 <= 0:
            raise ValueError(f"T_0={T_0!r}: a positive integer (epochs of the first cycle)")
        if isinstance(T_mult, bool) or not isinstance(T_mult, int) or T_mult < 1:
            raise ValueError(f"T_mult={T_mult!r}: an integer >= 1 (cycle length multiplier)")
        self.optim, self.T_0, self.T_i, self.T_mult, self.eta_min = optim, T_0, T_0, T_mult, float(eta_min)
        self.base_lr = optim.param_groups[0]["initial_lr"]
        self.T_cur = 0
        self.last_epoch = 0

    def get_last_lr(self):
        return [self.optim.param_groups[0]["lr"]]

    def step(self) -> None:
        self.last_epoch += 1
        self.T_cur += 1
        if self.T_cur >= self.T_i:
            self.T_cur -= self.T_i
            self.T_i *= self.T_mult
        self.optim.set_lr(self.eta_min + (self.base_lr - self.eta_min) * (1 + math.cos(math.pi * self.T_cur / self.T_i)) / 2)
