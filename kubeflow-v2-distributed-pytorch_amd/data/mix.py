"""Mixup / CutMix batch descriptors (timm's batch-mode ``Mixup`` semantics).

One training step mixes its batch with the batch's own reverse: sample ``i`` is paired with
sample ``B-1-i`` (timm's ``x.flip(0)``; no permutation tensor, and the middle sample of an odd
batch pairs with itself).  What the step does is a pure function of ``(seed, rank, epoch, step)``
written as eight fp32 values, the *descriptor*:

    [0] lambda: the weight of a sample's own label, in [0, 1]
    [1] mode:   0 none, 1 mixup, 2 cutmix
    [2..5]      y0, y1, x0, x1 of the CutMix box, half-open (small integers, exact in fp32)
    [6..7]      zero

The descriptor lives on the device: ``ops.kernels.batch_mix`` (csrc/kernels/mix.hip) and
``ops.functional.cross_entropy_mixed`` read it there, so nothing about a step is a host scalar and
a captured hipGraph replays with whatever the descriptor holds at that step.
"""
from __future__ import annotations

import math

import numpy as np
import torch

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2


def mix_params(seed: int, rank: int, epoch: int, step: int, H: int, W: int, *,
               mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
               switch_prob: float = 0.5) -> np.ndarray:
    """The descriptor (float32[8]) of step ``step`` of epoch ``epoch`` on rank ``rank``.

    * With probability ``1 - prob`` the step is not mixed: mode 0, lambda 1.
    * With both alphas > 0, CutMix is chosen with probability ``switch_prob``.
    * lambda ~ Beta(alpha, alpha) with the chosen mode's alpha.
    * CutMix: ``cut_h = int(H*sqrt(1-lambda))``, ``cut_w = int(W*sqrt(1-lambda))``, the centre
      uniform over the image, the box clipped to the image, and lambda recomputed as
      ``1 - area/(H*W)`` from the clipped integer box (1 for an empty box).

    Every random number comes from ``np.random.default_rng([seed, rank, epoch, step])``, drawn in
    a fixed order, so a step is the same across runs, across resume and between eager and graphed
    execution, and ranks draw independently."""
    out = np.zeros(8, np.float32)
    out[0] = 1.0
    if mixup_alpha <= 0.0 and cutmix_alpha <= 0.0:
        return out
    rng = np.random.default_rng([int(seed), int(rank), int(epoch), int(step)])
    u_apply, u_switch = rng.random(2)
    lam_mixup = float(rng.beta(mixup_alpha, mixup_alpha)) if mixup_alpha > 0.0 else 1.0
    lam_cutmix = float(rng.beta(cutmix_alpha, cutmix_alpha)) if cutmix_alpha > 0.0 else 1.0
    cy = int(rng.integers(0, H))
    cx = int(rng.integers(0, W))
    if not u_apply < prob:
        return out
    if mixup_alpha > 0.0 and cutmix_alpha > 0.0:
        cutmix = bool(u_switch < switch_prob)
    else:
        cutmix = cutmix_alpha > 0.0
    if not cutmix:
        out[0] = np.float32(min(max(lam_mixup, 0.0), 1.0))
        out[1] = MODE_MIXUP
        return out
    ratio = math.sqrt(max(0.0, 1.0 - lam_cutmix))
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    y0 = min(max(cy - cut_h // 2, 0), H)
    y1 = min(max(cy + cut_h // 2, 0), H)
    x0 = min(max(cx - cut_w // 2, 0), W)
    x1 = min(max(cx + cut_w // 2, 0), W)
    area = (y1 - y0) * (x1 - x0)
    out[0] = np.float32(1.0 - area / float(H * W))
    out[1] = MODE_CUTMIX
    out[2:6] = (y0, y1, x0, x1)
    return out


class BatchMixer:
    """Per-step descriptors on the device.

    Holds the options, pinned fp32[8] staging memory and ONE device fp32[8] tensor;
    :meth:`descriptor` computes the descriptor of ``(epoch, step)`` on the host and uploads it
    with one non-blocking 32-byte copy on the current stream: no host synchronisation and no
    device allocation per step.  The staging memory is a small ring of pinned slots, so the host
    may run ahead of the device by ``SLOTS - 1`` steps before it would have to wait for a slot's
    copy (an event per slot, checked only when the slot comes round again)."""

    SLOTS = 16

    def __init__(self, seed: int, rank: int, device, *, mixup_alpha: float = 0.0,
                 cutmix_alpha: float = 0.0, prob: float = 1.0, switch_prob: float = 0.5):
        self.seed, self.rank = int(seed), int(rank)
        self.device = torch.device(device)
        self.opts = dict(mixup_alpha=float(mixup_alpha), cutmix_alpha=float(cutmix_alpha),
                         prob=float(prob), switch_prob=float(switch_prob))
        self.enabled = mixup_alpha > 0.0 or cutmix_alpha > 0.0
        cuda = self.device.type == "cuda"
        self.staging = torch.zeros(self.SLOTS, 8, dtype=torch.float32, pin_memory=cuda)
        self.mix = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.mix[0] = 1.0
        self._events = [None] * self.SLOTS
        self._n = 0
        self.last = mix_params(0, 0, 0, 0, 1, 1)  # mode 0, lambda 1

    def params(self, epoch: int, step: int, H: int, W: int) -> np.ndarray:
        return mix_params(self.seed, self.rank, epoch, step, H, W, **self.opts)

    def descriptor(self, epoch: int, step: int, H: int, W: int) -> torch.Tensor:
        """The device descriptor, holding step ``(epoch, step)``'s values for everything queued
        on the current stream after this call (and until the next call)."""
        p = self.params(epoch, step, H, W)
        self.last = p
        k = self._n % self.SLOTS
        self._n += 1
        slot = self.staging[k]
        ev = self._events[k]
        if ev is not None:
            ev.synchronize()  # returns at once unless the host is SLOTS steps ahead
        slot.copy_(torch.from_numpy(p))
        self.mix.copy_(slot, non_blocking=True)
        if self.device.type == "cuda":
            if ev is None:
                ev = self._events[k] = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        return self.mix

    @property
    def last_mode(self) -> int:
        return int(self.last[1])

    @property
    def last_lambda(self) -> float:
        return float(self.last[0])
