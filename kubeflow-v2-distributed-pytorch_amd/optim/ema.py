"""Exponential moving average of the model weights on the flat buffer (``csrc/kernels/ema.hip``).

``ModelEMA`` keeps one fp32 copy of the model's flat parameter buffer and one of its floating-point
buffers (BatchNorm running statistics), the state torchvision's ``--model-ema`` and timm's
``ModelEmaV2`` average.  That is 4 B per parameter of extra memory; the average has no bf16 shadow
of its own.

* :meth:`ModelEMA.update` is three launches — the call counter's add and the two kernels — with
  no host value and no allocation: whether a call averages at all (``every``) and with which
  weight (the warm-up) is decided on the device from the counter, so the call can follow
  ``optimizer.step()`` inside a step captured into a hipGraph.
* :meth:`ModelEMA.swapped` exchanges live and averaged state IN PLACE (parameters, the bf16 shadow,
  float buffers) and exchanges it back on exit.  No pointer changes: the layers' shadow bindings,
  the DDP buckets, the prefetch order and captured graphs stay valid, and evaluation, export and
  checkpointing inside the context see the averaged model.

The averaging weight of call ``t`` (from 1), when ``t % every == 0``, with ``u = t/every − 1``::

    w = max(1 − decay, 9/(10 + u))   (warm-up; timm's decay_t = min(decay, (1+u)/(10+u)))
    w = 1 − decay                    (no warm-up)
    e = e + w·(p − e)

:func:`mipipe.ops._ref.ema_weight` / :func:`~mipipe.ops._ref.ema_update` are the contract and the
CPU path.  ``decay`` is used as given (torchvision rescales it by batch size and epochs: do that
in the caller if wanted).
"""
from __future__ import annotations

import contextlib
from typing import Any, Dict, List, Tuple

import torch

from mipipe.ops import _ref
from mipipe.ops import kernels as K
from .flat import FlatParamSpace, _view, flat_space_for

__all__ = ["ModelEMA", "ROW"]

ROW = 1024  # elements per buffer-table row (kEmaRowMax in csrc/kernels/launchers.hpp)


def _unwrap(model: torch.nn.Module) -> torch.nn.Module:
    from mipipe.parallel import DataParallel, DistributedDataParallel
    if isinstance(model, (DataParallel, torch.nn.DataParallel)):
        raise TypeError("ModelEMA does not support DataParallel: its replicas live outside the "
                        "master flat space; use DistributedDataParallel or a single device")
    if isinstance(model, (DistributedDataParallel, torch.nn.parallel.DistributedDataParallel)):
        return model.module
    return model


class ModelEMA:
    """``ModelEMA(model, decay=0.9999, every=1, warmup=True)``; ``model`` may be DDP-wrapped and
    must already have its optimizer (which builds the flat parameter space)."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, every: int = 1,
                 warmup: bool = True):
        self.module = _unwrap(model)
        params = list(self.module.parameters())
        if not params:
            raise ValueError("ModelEMA: the model has no parameters")
        owners = [flat_space_for(p) for p in params]
        if any(s is None for s in owners) or len({id(s) for s in owners}) != 1:
            raise RuntimeError("ModelEMA: every parameter of the model must belong to one "
                               "FlatParamSpace (create the mipipe optimizer first)")
        self.space: FlatParamSpace = owners[0]
        self._set_hparams(decay, every, warmup)
        flat = self.space.flat
        dev = flat.device
        self.ema = flat.detach().clone()
        self._t_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._scal = torch.zeros(4, dtype=torch.float32, device=dev)
        # float buffers: owners are remembered as (module, name) because DDP re-homes the tensors
        # themselves into one flat tensor at its first forward (ddp.py::_flatten_buffers)
        self._owners: List[Tuple[torch.nn.Module, str]] = []
        self._slots: Dict[str, Tuple[int, int]] = {}  # state_dict name -> (offset, numel)
        off = 0
        seen = set()
        for mname, mod in self.module.named_modules():
            for bname, b in mod._buffers.items():
                if b is None or not b.is_floating_point():
                    continue
                if id(b) in seen:
                    # one tensor under two names would need one slot and two state_dict keys;
                    # no model here does that, and averaging it twice would be wrong
                    raise ValueError(f"ModelEMA: buffer {mname}.{bname} is registered twice")
                seen.add(id(b))
                if b.dtype != torch.float32 or b.device != dev:
                    raise ValueError(f"ModelEMA: buffer {mname}.{bname} must be fp32 on {dev}, "
                                     f"got {b.dtype} on {b.device}")
                self._owners.append((mod, bname))
                self._slots[f"{mname}.{bname}" if mname else bname] = (off, b.numel())
                off += b.numel()
        self._offs = [o for o, _ in self._slots.values()]
        self.ema_buffers = torch.zeros(max(off, 1), dtype=torch.float32, device=dev)
        self._nbuf = off
        self._copy_buffers_in()
        self._native = K.use_native(flat)
        if self._native and K.native().EMA_ROW_MAX != ROW:
            raise RuntimeError("mipipe._C was built with another EMA row size; rebuild it")
        self._ptrs: List[int] = []
        self._table = None  # device int64 [rows, 3], built at the first eager call
        self._in_swap = False

    def _set_hparams(self, decay: float, every: int, warmup: bool) -> None:
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("ModelEMA: decay must lie in [0, 1)")
        if int(every) < 1:
            raise ValueError("ModelEMA: every must be >= 1")
        self.decay, self.every, self.warmup = float(decay), int(every), bool(warmup)
        # 1 - decay in double, rounded once to fp32: the kernel's w_min
        self._w_min = float(torch.tensor(1.0 - self.decay, dtype=torch.float64).float())

    # ------------------------------------------------------------------ buffers
    def _buffers(self) -> List[torch.Tensor]:
        return [mod._buffers[name] for mod, name in self._owners]

    def _buffer_views(self) -> List[torch.Tensor]:
        return [self.ema_buffers[o:o + b.numel()].view_as(b)
                for o, b in zip(self._offs, self._buffers())]

    def _copy_buffers_in(self) -> None:
        for b, v in zip(self._buffers(), self._buffer_views()):
            v.copy_(b.detach())

    def _settle_table(self) -> None:
        """Make the device table point at the buffers' current storage.  Only in eager mode:
        during capture the addresses are those of the eager step that preceded it."""
        if not self._native or not self._owners:
            return
        if torch.cuda.is_current_stream_capturing():
            if self._table is None:
                raise RuntimeError("ModelEMA: call update() once eagerly before capturing it "
                                   "(GraphedStep's warm-up step does)")
            return
        bufs = self._buffers()
        ptrs = [b.data_ptr() for b in bufs]
        if ptrs == self._ptrs:
            return
        rows = []
        for b, p, o in zip(bufs, ptrs, self._offs):
            if not b.is_contiguous() or p % 4:
                raise ValueError("ModelEMA: float buffers must be contiguous and 4-byte aligned")
            for s in range(0, b.numel(), ROW):
                rows.append((p + 4 * s, o + s, min(ROW, b.numel() - s)))
        host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)
        assert int((host[:, 1] + host[:, 2]).max()) <= self._nbuf
        if self._table is None:
            self._table = host.to(self.ema.device)
        else:  # in place: a captured step reads this very tensor (the row count never changes)
            self._table.copy_(host)
        self._ptrs = ptrs

    # ------------------------------------------------------------------ update / swap
    @torch.no_grad()
    def update(self) -> None:
        """Count one call and, every ``every``-th call, average.  Call it after
        ``optimizer.step()``; capturable."""
        self._settle_table()
        self._t_dev.add_(1)
        K.ema_update(self.space.flat, self.ema, self._t_dev, self.every, self._w_min, self.warmup,
                     self._scal)
        if not self._owners:
            return
        if self._native:
            K.ema_buffers_update(self._table, self.ema_buffers, self._t_dev, self.every,
                                 self._w_min, self.warmup)
        else:
            w = _ref.ema_weight(int(self._t_dev.item()), self.every, self._w_min, self.warmup)
            if w is not None:
                for b, v in zip(self._buffers(), self._buffer_views()):
                    _ref.ema_update(v, b, w)

    @torch.no_grad()
    def _swap(self) -> None:
        self._settle_table()
        K.ema_swap(self.space.flat, self.ema, self.space.shadow)
        if self._owners:
            if self._native:
                K.ema_buffers_swap(self._table, self.ema_buffers)
            else:
                for b, v in zip(self._buffers(), self._buffer_views()):
                    _ref.ema_swap(b, v)
        self.space.mark_synced()

    @contextlib.contextmanager
    def swapped(self):
        """Inside the context the model holds the averaged parameters, shadow and float buffers
        and this object holds the live ones; on exit they are exchanged back bit for bit."""
        if self._in_swap:
            raise RuntimeError("ModelEMA.swapped() is already active")
        self._in_swap = True
        self._swap()
        try:
            yield self
        finally:
            self._swap()
            self._in_swap = False

    # ------------------------------------------------------------------ inspection / state
    def last_weight(self) -> torch.Tensor:
        """The weight the last averaging update used, as computed on the device (0-d tensor)."""
        return self._scal[0]

    def num_calls(self) -> int:
        """``update()`` calls so far (synchronises: after graph replays only the device knows)."""
        return int(self._t_dev.item())

    def num_updates(self) -> int:
        """Averaging updates so far: ``num_calls() // every``."""
        return self.num_calls() // self.every

    def _check_not_swapped(self, what: str) -> None:
        if self._in_swap:
            raise RuntimeError(f"ModelEMA.{what} inside swapped(): the roles are exchanged there; "
                               "use the model's own state_dict()")

    def module_state_dict(self) -> Dict[str, torch.Tensor]:
        """The averaged model as a ``state_dict`` of the unwrapped module: the same keys (no
        ``module.`` prefix) and shapes; integer buffers (``num_batches_tracked``) are the live
        ones.  Detached copies."""
        self._check_not_swapped("module_state_dict()")
        out: Dict[str, torch.Tensor] = {}
        views = dict(zip(self._slots, self._buffer_views()))
        for k, v in self.module.state_dict(keep_vars=True).items():
            if id(v) in self.space.offsets:
                out[k] = _view(self.ema, self.space.offsets[id(v)], v).detach().clone()
            elif k in views:
                out[k] = views[k].detach().clone()
            else:
                out[k] = v.detach().clone()
        return out

    def state_dict(self) -> Dict[str, Any]:
        """``{'model': averaged module state_dict, 'calls', 'decay', 'every', 'warmup'}`` — tensors
        and primitives only (loads with ``weights_only=True``)."""
        return {"model": self.module_state_dict(), "calls": self.num_calls(),
                "decay": self.decay, "every": self.every, "warmup": self.warmup}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """In place (a captured step goes on working); ``decay`` / ``every`` / ``warmup`` are
        launch arguments, so load before capturing."""
        self._check_not_swapped("load_state_dict()")
        src = {(k[len("module."):] if k.startswith("module.") else k): v
               for k, v in sd["model"].items()}
        views = dict(zip(self._slots, self._buffer_views()))
        live = self.module.state_dict(keep_vars=True)
        missing = [k for k in live if k not in src]
        if missing:
            raise KeyError(f"ModelEMA.load_state_dict: missing keys {missing[:5]}")
        for k, v in live.items():
            if id(v) in self.space.offsets:
                _view(self.ema, self.space.offsets[id(v)], v).copy_(src[k].reshape(v.shape))
            elif k in views:
                views[k].copy_(src[k].reshape(views[k].shape))
        self._set_hparams(sd["decay"], sd["every"], sd["warmup"])
        self._t_dev.fill_(int(sd["calls"]))

    @torch.no_grad()
    def reset(self) -> None:
        """Start over from the model's current weights, in place."""
        self._check_not_swapped("reset()")
        self.ema.copy_(self.space.flat)
        self._copy_buffers_in()
        self._t_dev.zero_()
        self._scal.zero_()
