"""Evaluation metrics accumulated on the device: top-1 / top-k accuracy, cross-entropy, expected
calibration error, a confidence curve and the confusion matrix with its per-class figures.

:class:`EvalMeter` owns the integer buffers that ``eval_stats`` (csrc/kernels/eval_stats.hip; the
contract is :func:`mipipe.ops._ref.eval_stats`) adds to: one launch per batch, no host sync, one
all-reduce per evaluation and one device-to-host read in :meth:`EvalMeter.result`.  Every sum is an
integer (loss and confidence in Q24 fixed point), so the figures do not depend on how the rows were
split over batches or ranks.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .ops import kernels as K

__all__ = ["EvalMeter", "derive_metrics", "CONFUSION_MAX_CLASSES"]

_Q24 = float(1 << 24)
_NCOUNT = 8  # rows, top1, topk, nonfinite, invalid, loss_q24, 0, 0
CONFUSION_MAX_CLASSES = 4096  # task.py allocates the confusion matrix up to this many classes


def derive_metrics(counters, hist=None, confusion=None, topk: int = 5) -> Dict:
    """The result dict from the raw sums (host tensors or nested lists): ``counters`` int64 [8],
    ``hist`` int64 [3, bins] or None, ``confusion`` [C, C] (rows: labels, columns: predictions) or
    None.  A ratio with a zero denominator is 0, and such a class is left out of the macro means."""
    c = [int(v) for v in torch.as_tensor(counters).reshape(-1).tolist()]
    rows, top1, topk_hits, nonfinite, invalid, loss_q = c[:6]
    finite = rows - nonfinite
    out = {"rows": rows,
           "accuracy": float(top1) / max(1, rows),
           f"accuracy_top{topk}": float(topk_hits) / max(1, rows),
           "loss": (loss_q / _Q24) / finite if finite > 0 else 0.0,
           "nonfinite": nonfinite, "invalid": invalid}
    if hist is not None:
        h = torch.as_tensor(hist).to(torch.int64).cpu()
        bins = h.shape[1]
        wrong, right = h[0].tolist(), h[1].tolist()
        conf = [v / _Q24 for v in h[2].tolist()]
        n = sum(wrong) + sum(right)
        ece = 0.0
        for b in range(bins):
            nb = wrong[b] + right[b]
            if nb:
                ece += nb / n * abs(right[b] / nb - conf[b] / nb)
        out["ece"] = ece
        curve: List = []
        cnt = ok = 0
        for b in range(bins - 1, -1, -1):  # rows with conf >= b / bins: bins b .. bins-1
            cnt += wrong[b] + right[b]
            ok += right[b]
            curve.append((b / bins, cnt / n if n else 0.0, ok / cnt if cnt else 0.0))
        out["confidence_curve"] = curve[::-1]
    if confusion is not None:
        cm = torch.as_tensor(confusion).to(torch.int64).cpu()
        tp = cm.diag().double()
        support = cm.sum(1)
        predicted = cm.sum(0)
        both = support + predicted

        def ratio(num, den):
            return torch.where(den > 0, num / den.clamp_min(1).double(), torch.zeros_like(num))

        recall, precision, f1 = ratio(tp, support), ratio(tp, predicted), ratio(2 * tp, both)
        def macro(v, seen):  # mean over the classes that have a denominator
            return float(v[seen].mean()) if bool(seen.any()) else 0.0

        out.update(confusion=cm.tolist(), recall=recall.tolist(), precision=precision.tolist(),
                   f1=f1.tolist(), support=support.tolist(),
                   balanced_accuracy=macro(recall, support > 0), macro_f1=macro(f1, both > 0))
    return out


class EvalMeter:
    """Accumulates evaluation statistics on ``device``.

    ``num_classes``: width of the logits; ``valid_cols`` (``0 < valid_cols < num_classes``): only
    the first columns are classes (a vocabulary padded to a tile width).  ``topk`` is clamped to
    the class count.  ``bins``: confidence bins of the histogram (1..64).  ``confusion=False``
    leaves the ``[classes, classes]`` matrix out (large vocabularies)."""

    def __init__(self, num_classes: int, topk: int = 5, bins: int = 15, confusion: bool = True,
                 ignore_index: int = -100, valid_cols: int = -1, device="cpu"):
        if num_classes < 1:
            raise ValueError("num_classes must be >= 1")
        if not 1 <= bins <= 64:
            raise ValueError(f"bins must be in [1, 64], got {bins}")
        self.num_classes = int(num_classes)
        self.valid_cols = int(valid_cols)
        padded = 0 < self.valid_cols < self.num_classes
        self.classes = self.valid_cols if padded else self.num_classes
        self.topk = max(1, min(int(topk), self.classes))
        self.bins = int(bins)
        self.ignore_index = int(ignore_index)
        self.device = torch.device(device)
        # counters and histogram share one allocation: one all-reduce, one read
        self._state = torch.zeros(_NCOUNT + 3 * self.bins, dtype=torch.int64, device=self.device)
        self.counters = self._state[:_NCOUNT]
        self.hist = self._state[_NCOUNT:].view(3, self.bins)
        self.confusion = (torch.zeros(self.classes, self.classes, dtype=torch.int32,
                                      device=self.device) if confusion else None)

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        """One ``eval_stats`` call on logits ``[R, num_classes]`` (fp32 / bf16) and int64 labels."""
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"logits must be [R, {self.num_classes}], got {tuple(logits.shape)}")
        K.eval_stats(logits, labels.reshape(-1), self.counters, self.confusion, self.hist,
                     self.topk, self.ignore_index, self.valid_cols)

    def all_reduce(self) -> None:
        """Sum the buffers over the process group (gloo or RCCL) with one all-reduce; the int32
        confusion matrix travels as int64.  A no-op without a group or at world size 1."""
        dist = torch.distributed
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        if self.confusion is None:
            dist.all_reduce(self._state)
            return
        wire = torch.cat([self._state, self.confusion.reshape(-1).to(torch.int64)])
        dist.all_reduce(wire)
        n = self._state.numel()
        self._state.copy_(wire[:n])
        self.confusion.copy_(wire[n:].view_as(self.confusion))

    def result(self) -> Dict:
        """The metrics dict (:func:`derive_metrics`) after the single device-to-host read."""
        if self.confusion is None:
            host = self._state.cpu()
            cm = None
        else:
            # one int32 transfer: the int64 sums travel as pairs of words beside the int32 matrix
            wire = torch.cat([self._state.view(torch.int32), self.confusion.reshape(-1)]).cpu()
            n = 2 * self._state.numel()
            host = wire[:n].view(torch.int64)
            cm = wire[n:].view(self.classes, self.classes)
        hist = host[_NCOUNT:_NCOUNT + 3 * self.bins].view(3, self.bins)
        return derive_metrics(host[:_NCOUNT], hist, cm, self.topk)

    def log_to(self, classification_metrics, categories: Optional[List[str]] = None,
               result: Optional[Dict] = None) -> Dict:
        """Fill a ``ClassificationMetrics`` artifact: the confusion matrix (when it is on) and one
        ``confidenceMetrics`` point per curve point, with ``confidenceThreshold`` the threshold,
        ``recall`` the share of rows at or above it and ``falsePositiveRate`` 1 - the accuracy
        among those rows.  Returns the result dict it used."""
        res = result if result is not None else self.result()
        if "confusion" in res:
            cats = [str(i) for i in range(self.classes)] if categories is None else list(categories)
            classification_metrics.log_confusion_matrix(cats, res["confusion"])
        for thr, share, acc in res["confidence_curve"]:
            classification_metrics.log_roc_data_point(1.0 - acc, share, thr)
        return res

    def reset(self) -> None:
        """Zero the buffers in place (their addresses stay, as a captured graph needs)."""
        self._state.zero_()
        if self.confusion is not None:
            self.confusion.zero_()
