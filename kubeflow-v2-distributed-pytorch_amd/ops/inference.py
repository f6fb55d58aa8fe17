"""Fused evaluation: the eval-mode tail of a conv block in the conv's own epilogue.

In eval mode BatchNorm is a fixed per-channel affine, known before the conv starts.  With the
switch on, ``nn.conv_bn_act`` and the model zoo's ``conv_bn`` run conv -> BN -> [+residual] ->
[ReLU] as ONE launch of the inference conv (csrc/kernels/conv_infer.hip) plus one small launch
that folds the BN's running statistics (and a conv bias) into (scale, shift): the conv output
is never written un-normalised, the separate BN-apply pass and its four ATen ops disappear.

It applies only where nothing can need a backward: the BN in eval mode and autograd off.
Training, grad-enabled evaluation, grouped / depthwise convs, ReLU6 and the packed ResNet stem
keep their usual path.  Off by default; ``MIPIPE_FUSED_EVAL=1`` turns it on at import.
"""
from __future__ import annotations

import contextlib
import os

__all__ = ["set_fused_eval", "is_fused_eval", "fused_eval"]

_FUSED_EVAL = os.environ.get("MIPIPE_FUSED_EVAL", "0") == "1"


def set_fused_eval(on: bool = True) -> None:
    global _FUSED_EVAL
    _FUSED_EVAL = bool(on)


def is_fused_eval() -> bool:
    return _FUSED_EVAL


@contextlib.contextmanager
def fused_eval(on: bool = True):
    old = is_fused_eval()
    set_fused_eval(on)
    try:
        yield
    finally:
        set_fused_eval(old)
