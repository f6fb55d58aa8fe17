"""Large-batch optimizers on the flat buffer: ``LARS`` (vision) and ``LAMB`` (BERT), with
global-norm gradient clipping and a learning-rate schedule evaluated ON THE DEVICE.

Every per-step scalar — the step count, the step's learning rate, the clip coefficient, the
per-parameter trust ratios — lives in device memory and is produced by the step's own kernels
(``csrc/kernels/optim.hip``), so a step captured into a hipGraph (``train/graph.py``) replays with
the right learning rate every time.  A step is 3 launches (LAMB with clipping: 5):

* a norm pass, one block per *chunk* of the flat buffer (at most ``CHUNK`` elements, never
  crossing a parameter's segment), writing per-chunk partial sums of squares;
* ``seg_finish``, one block: per-segment norms, the global gradient norm, clip, trust ratios, LR;
* the apply pass, one block per chunk, which also rewrites the bf16 shadow.

The update rules are :func:`mipipe.ops._ref.lars_step` / :func:`~mipipe.ops._ref.lamb_step`
(per tensor; they are also the CPU path).  ``LARS(trust_coefficient=None)`` is the project's
momentum SGD with a device LR and clipping.

Under DDP nothing changes: the step runs after the reduced gradients are in place, so every rank
computes identical norms.  ``DataParallel`` sums the replicas' gradients into the master flat
space before the step, which is all these optimizers read, so they run through it unchanged.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops._native import native
from . import _FlatOptimizer  # the package module imports this one after defining it

__all__ = ["LARS", "LAMB", "LRSchedule", "CHUNK", "build_tables"]

CHUNK = 8192  # elements per chunk (kOptimChunk in csrc/kernels/launchers.hpp)
_ALIGN = 64
KINDS = ("constant", "linear", "poly", "cosine")


class LRSchedule:
    """Warm-up then decay.  Step ``k`` counts from 0; with W = ``warmup_steps``, T =
    ``total_steps`` and ``x = (k − W)/(T − W)`` clamped to [0, 1]:

    * ``k < W``: ``base·(k+1)/W``;
    * ``constant``: ``base``; ``linear``: ``end + (base−end)(1−x)``; ``poly``:
      ``end + (base−end)(1−x)²``; ``cosine``: ``end + (base−end)·½(1+cos πx)``.

    :meth:`lr_at` is the host twin (double precision) of what ``seg_finish`` computes from the
    device step counter."""

    def __init__(self, kind: str = "constant", base_lr: float = 0.1, warmup_steps: int = 0,
                 total_steps: int = 0, end_lr: float = 0.0):
        if kind not in KINDS:
            raise ValueError(f"LR schedule kind must be one of {KINDS}, got '{kind}'")
        if warmup_steps < 0 or total_steps < 0:
            raise ValueError("warmup_steps and total_steps must be >= 0")
        self.kind, self.base_lr, self.end_lr = kind, float(base_lr), float(end_lr)
        self.warmup_steps, self.total_steps = int(warmup_steps), int(total_steps)

    def lr_at(self, k: int) -> float:
        return _ref.lr_schedule(self.kind, self.base_lr, self.warmup_steps, self.total_steps,
                                self.end_lr, int(k))

    def group(self) -> Dict[str, Any]:
        """The schedule as param-group entries (``lr`` is the base learning rate)."""
        return dict(lr=self.base_lr, lr_schedule=self.kind, warmup_steps=self.warmup_steps,
                    total_steps=self.total_steps, end_lr=self.end_lr)

    @classmethod
    def from_group(cls, g: Dict[str, Any]) -> "LRSchedule":
        return cls(g["lr_schedule"], g["lr"], g["warmup_steps"], g["total_steps"], g["end_lr"])


def build_tables(ranges: Sequence[Tuple[int, int]], weight_decay: Sequence[float],
                 adapt: Sequence[bool]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Chunk and segment tables of a flat space (CPU int32 tensors, uploaded once).

    ``ranges``: each segment's reserved ``(start, end)`` in flat order (alignment padding and
    reserved pad rows included).  Chunks ``[nchunks, 4] = (segment, start // 64, length, 0)`` tile
    every segment exactly once, in order, in pieces of at most ``CHUNK`` elements, none crossing a
    segment; segments ``[nseg, 4] = (weight decay as float bits, adapt, first chunk, chunks)``."""
    chunks: List[Tuple[int, int, int, int]] = []
    first, count = [], []
    for s, (a, b) in enumerate(ranges):
        if a % _ALIGN or b % _ALIGN or b <= a:
            raise ValueError(f"segment {s} [{a}, {b}) is not a non-empty 64-aligned range")
        first.append(len(chunks))
        for o in range(a, b, CHUNK):
            chunks.append((s, o // _ALIGN, min(CHUNK, b - o), 0))
        count.append(len(chunks) - first[-1])
    segs = torch.zeros(len(first), 4, dtype=torch.int32)
    segs[:, 0] = torch.tensor(list(weight_decay), dtype=torch.float32).view(torch.int32)
    segs[:, 1] = torch.tensor([int(bool(a)) for a in adapt], dtype=torch.int32)
    segs[:, 2] = torch.tensor(first, dtype=torch.int32)
    segs[:, 3] = torch.tensor(count, dtype=torch.int32)
    return torch.tensor(chunks, dtype=torch.int32).reshape(-1, 4), segs


class _LargeBatch(_FlatOptimizer):
    """Shared machinery: schedule and step count in the param group, device tables, device step
    counter, clipping, the CPU per-tensor path."""

    _state_names: List[str] = []

    def __init__(self, params, defaults: Dict[str, Any], lr: Union[float, LRSchedule],
                 max_grad_norm: Optional[float], exclude_1d: bool, shadow_dtype):
        sched = lr if isinstance(lr, LRSchedule) else LRSchedule("constant", float(lr))
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be positive (None turns clipping off)")
        defaults = dict(defaults, **sched.group(), max_grad_norm=max_grad_norm,
                        exclude_1d=bool(exclude_1d), step=0)
        super().__init__(params, defaults, shadow_dtype)
        flat = self.space.flat
        self._step = 0
        # the step count lives on the device (int32 [1]) and a device op advances it: a captured
        # step derives its LR (and LAMB's bias corrections) from it on every replay
        self.device_step = flat.is_cuda
        if K.use_native(flat) and native().OPTIM_CHUNK != CHUNK:
            raise RuntimeError("mipipe._C was built with another optimizer chunk size; rebuild it")
        self._t_dev = torch.zeros(1, dtype=torch.int32, device=flat.device) if self.device_step \
            else None
        self._order = list(self.space.order)  # segment s is parameter _order[s]
        nseg = len(self._order)
        self._segs = self._chunks = None
        self._upload_tables()
        nchunks = self._chunks.shape[0]
        dev = flat.device
        self._part = torch.zeros(2 * nchunks, dtype=torch.float32, device=dev)
        self._segtot = torch.zeros(2 * nseg, dtype=torch.float32, device=dev)
        self._ratio = torch.ones(nseg, dtype=torch.float32, device=dev)
        self._scal = torch.tensor([sched.lr_at(0), 1.0, 0.0, 0.0], dtype=torch.float32, device=dev)
        self._have_norm = False
        for n in self._state_names:
            self._flat_state(n)
        self._per_param_state(self._state_names)

    # ------------------------------------------------------------------ tables
    def _adapts(self, g) -> bool:
        return True

    def _seg_params(self) -> Tuple[List[float], List[bool]]:
        """Per-segment (weight decay, adapt).  ``exclude_1d``: biases, BN / LayerNorm affine
        parameters (``dim() <= 1``) take no decay and ratio 1."""
        g = self.param_groups[0]
        wd, ad = [], []
        for p in self._order:
            skip = g["exclude_1d"] and p.dim() <= 1
            wd.append(0.0 if skip else float(g["weight_decay"]))
            ad.append(self._adapts(g) and not skip)
        return wd, ad

    def _upload_tables(self) -> None:
        wd, ad = self._seg_params()
        chunks, segs = build_tables([(a, b) for a, b, _ in self.space.ranges()], wd, ad)
        top = int((chunks[:, 1].long() * _ALIGN + chunks[:, 2]).max())
        assert top <= self.space.numel and int(chunks[:, 0].max()) < segs.shape[0]
        if self._chunks is None:
            self._chunks = chunks.to(self.space.flat.device)
            self._segs = segs.to(self.space.flat.device)
        else:  # in place: a captured step reads these very tensors
            self._segs.copy_(segs)

    # ------------------------------------------------------------------ schedule / step count
    @property
    def schedule(self) -> LRSchedule:
        return LRSchedule.from_group(self.param_groups[0])

    def sync_step(self) -> int:
        """Host view of the step count (after graph replays the device counter is ahead)."""
        if self._t_dev is not None:
            self._step = int(self._t_dev.item())
        self.param_groups[0]["step"] = self._step
        return self._step

    def current_lr(self) -> float:
        """``lr_at(sync_step())``: the learning rate of the step about to be taken."""
        return self.schedule.lr_at(self.sync_step())

    def last_lr(self) -> torch.Tensor:
        """The learning rate the last step used, as computed on the device (0-d tensor)."""
        return self._scal[0]

    def last_trust_ratios(self) -> torch.Tensor:
        """Trust ratios of the last step, one per parameter in flat order (``space.order``); a
        device tensor: reading it synchronises, asking for it does not."""
        return self._ratio

    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Global norm of ``grad · grad_scale`` at the last step (0-d device tensor), or None when
        that step computed no gradient norm (LAMB without clipping, LARS with neither ratio nor
        clipping)."""
        return self._scal[2] if self._have_norm else None

    def state_dict(self):
        self.sync_step()
        return super().state_dict()

    def _after_load(self) -> None:
        self._step = int(self.param_groups[0].get("step", 0))
        if self._t_dev is not None:
            self._t_dev.fill_(self._step)
        self._upload_tables()  # weight decay / exclude_1d may have changed with the group

    def reset_state(self) -> None:
        super().reset_state()
        self._step = 0
        self.param_groups[0]["step"] = 0
        if self._t_dev is not None:
            self._t_dev.zero_()  # in place: captured steps advance this very tensor

    # ------------------------------------------------------------------ step
    def _sched_args(self, g) -> Tuple[int, float, float, int, int]:
        return (KINDS.index(g["lr_schedule"]), float(g["lr"]), float(g["end_lr"]),
                int(g["warmup_steps"]), int(g["total_steps"]))

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        self._step += 1
        if K.use_native(self.space.flat):
            self._t_dev.add_(1)
            self._native_step(g, float(grad_scale))
        else:
            self._cpu_step(g, float(grad_scale))
        self.space.mark_synced()
        return loss

    def _native_step(self, g, grad_scale: float) -> None:
        raise NotImplementedError

    def _one(self, g, s: int, p: torch.Tensor, grad: torch.Tensor, lr: float, gsc, wd: float,
             adapt: bool) -> torch.Tensor:
        raise NotImplementedError

    def _cpu_step(self, g, grad_scale: float) -> None:
        """The ``_ref`` rules per tensor, in fp32 (no ``_C``: CPU suite, gloo DDP)."""
        lr = self.schedule.lr_at(self._step - 1)
        grads = [self.space.grad_view(p) for p in self._order]
        gsc: Any = grad_scale
        self._have_norm = self._wants_norm(g)
        if self._have_norm:
            norm, clip = _ref.clip_coef(grads, grad_scale, g["max_grad_norm"])
            self._scal[1], self._scal[2] = clip, norm
            gsc = grad_scale * clip
        wds, ads = self._seg_params()
        for s, p in enumerate(self._order):
            self._ratio[s] = self._one(g, s, p, grads[s], lr, gsc, wds[s], ads[s])
        self._scal[0] = lr
        if self.space.shadow is not None:
            self.space.shadow.copy_(self.space.flat)

    def _wants_norm(self, g) -> bool:
        return g["max_grad_norm"] is not None


class LARS(_LargeBatch):
    """Layer-wise adaptive rate scaling over momentum SGD (LARC-style composition)::

        r = tc·‖w‖ / (‖g'‖ + wd·‖w‖ + eps)   (1 if not adapted or a norm is 0)
        d = r·(g' + wd·w);  m = μ·m + d;  w −= lr·m          g' = g · grad_scale · clip

    ``lr``: a float or an :class:`LRSchedule`.  ``trust_coefficient=None``: r = 1 everywhere —
    the project's momentum SGD with a device-side LR and clipping.  ``exclude_1d``: parameters
    with ``dim() <= 1`` take ratio 1 and no weight decay."""

    _state_names = ["momentum_buffer"]

    def __init__(self, params, lr: Union[float, LRSchedule] = 0.1, momentum: float = 0.9,
                 weight_decay: float = 0.0, trust_coefficient: Optional[float] = 0.001,
                 eps: float = 1e-8, max_grad_norm: Optional[float] = None,
                 exclude_1d: bool = True, shadow_dtype="auto"):
        if trust_coefficient is not None and not trust_coefficient > 0:
            raise ValueError("trust_coefficient must be positive (None: no trust ratio)")
        defaults = dict(momentum=momentum, weight_decay=weight_decay,
                        trust_coefficient=trust_coefficient, eps=eps)
        super().__init__(params, defaults, lr, max_grad_norm, exclude_1d, shadow_dtype)

    def _adapts(self, g) -> bool:
        return g["trust_coefficient"] is not None

    def _wants_norm(self, g) -> bool:
        return g["max_grad_norm"] is not None or g["trust_coefficient"] is not None

    def _native_step(self, g, grad_scale: float) -> None:
        tc, mx = g["trust_coefficient"], g["max_grad_norm"]
        self._have_norm = self._wants_norm(g)
        native().lars_step(self.space.flat, self.space.flat_grad,
                           self._flat_state("momentum_buffer"), self.space.shadow, self._chunks,
                           self._segs, self._part, self._segtot, self._ratio, self._scal,
                           self._t_dev, float(g["momentum"]), -1.0 if tc is None else float(tc),
                           float(g["eps"]), 0.0 if mx is None else float(mx), grad_scale,
                           *self._sched_args(g))

    def _one(self, g, s, p, grad, lr, gsc, wd, adapt):
        return _ref.lars_step(p.data, grad, self.state[p]["momentum_buffer"], lr,
                              float(g["momentum"]), wd, g["trust_coefficient"], float(g["eps"]),
                              adapt, gsc)


class LAMB(_LargeBatch):
    """Layer-wise adaptive moments (You et al.)::

        m = β1·m + (1−β1)·g';  v = β2·v + (1−β2)·g'²         g' = g · grad_scale · clip
        u = (m/(1−β1ᵗ)) / (√(v/(1−β2ᵗ)) + eps) + wd·w
        r = ‖w‖/‖u‖   (1 if not adapted or a norm is 0);      w −= lr·r·u

    ``t`` is the device step count.  The apply pass recomputes ``u`` from (w, m, v), so the
    gradient buffer is left intact by ``step()``."""

    _state_names = ["exp_avg", "exp_avg_sq"]

    def __init__(self, params, lr: Union[float, LRSchedule] = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-6, weight_decay: float = 0.01,
                 max_grad_norm: Optional[float] = None, exclude_1d: bool = True,
                 shadow_dtype="auto"):
        b1, b2 = betas
        if not (0.0 < b1 < 1.0 and 0.0 < b2 < 1.0):
            raise ValueError("LAMB betas must lie in (0, 1)")
        defaults = dict(betas=(float(b1), float(b2)), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults, lr, max_grad_norm, exclude_1d, shadow_dtype)

    def sync_step(self) -> int:
        n = super().sync_step()
        for p in self.params:  # torch.optim.Adam's per-parameter ``step``
            self.state[p]["step"] = torch.tensor(float(n))
        return n

    def _native_step(self, g, grad_scale: float) -> None:
        b1, b2 = g["betas"]
        mx = g["max_grad_norm"]
        self._have_norm = mx is not None
        native().lamb_step(self.space.flat, self.space.flat_grad, self._flat_state("exp_avg"),
                           self._flat_state("exp_avg_sq"), self.space.shadow, self._chunks,
                           self._segs, self._part, self._segtot, self._ratio, self._scal,
                           self._t_dev, float(b1), float(b2), float(g["eps"]),
                           0.0 if mx is None else float(mx), grad_scale, *self._sched_args(g))

    def _one(self, g, s, p, grad, lr, gsc, wd, adapt):
        b1, b2 = g["betas"]
        st = self.state[p]
        return _ref.lamb_step(p.data, grad, st["exp_avg"], st["exp_avg_sq"], lr, float(b1),
                              float(b2), float(g["eps"]), wd, self._step, adapt, gsc)
