"""EfficientNet b0 ... b7 (torchvision layout) on mipipe's NHWC kernels.

An MBConv block is a 1x1 expansion, a depthwise 3x3 / 5x5 at stride 1 / 2, BatchNorm + SiLU,
squeeze-excitation with a sigmoid gate and a 1x1 projection.  The expansion and projection run on
the MFMA implicit-GEMM conv with BatchNorm statistics in its epilogue; the depthwise conv is
``dwconvk.hip``'s halo-resident kernel, whose forward also produces the BatchNorm statistics
(:func:`mipipe.models._zoo.dwconv_bn_act_pool`); BatchNorm + SiLU is ``se.hip``'s ``bn_act_pool``
(SiLU's derivative cannot be read from its output: the backward recomputes the pre-activation),
with the SE squeeze from the same pass; the two SE FCs are 1x1 convolutions on the pooled
``[N, 1, 1, C]`` tensor and ``se_scale(..., "sigmoid")`` multiplies the gate back.  A residual
block closes with the projection's BatchNorm apply taking the residual, or — in training with
stochastic depth ("row" mode, torchvision's default 0.2 spread linearly over the blocks) — with
:func:`mipipe.ops.functional.scale_residual` and a constant-one scale; the keep mask of block i is
the dropout hash of (seed of the site and step, sample index), the per-step part a device counter
on the GPU, so a captured step draws a new mask on every replay.  ``state_dict`` keys and shapes
follow torchvision (``features.2.0.block.2.fc1.weight``, ``classifier.1.weight`` ...).
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K

from . import register_model
from ._zoo import (ZooModel, conv_bn, dwconv_bn_act_pool, dwconvk_route, global_pool, ref_linear,
                   run_seq)
from .convnext import _seed
from .mobilenet import _make_divisible

__all__ = ["EfficientNet", "MBConv"] + [f"efficientnet_b{i}" for i in range(8)]

#: (expand ratio, kernel, stride, input channels, output channels, layers) of the b0 stages
_STAGES = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3),
           (6, 5, 1, 80, 112, 3), (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1))
#: (width multiplier, depth multiplier, dropout) of b0 ... b7
_VARIANTS = ((1.0, 1.0, 0.2), (1.0, 1.1, 0.2), (1.1, 1.2, 0.3), (1.2, 1.4, 0.3), (1.4, 1.8, 0.4),
             (1.6, 2.2, 0.4), (1.8, 2.6, 0.5), (2.0, 3.1, 0.5))


def _conv_bn_act(cin: int, cout: int, kernel: int, stride: int, groups: int, eps: float,
                 momentum: float, act: bool = True) -> tnn.Sequential:
    """torchvision's Conv2dNormActivation: conv (no bias), BatchNorm, SiLU."""
    layers: List[tnn.Module] = [
        mnn.XConv2d(cin, cout, kernel, stride, (kernel - 1) // 2, groups=groups, bias=False),
        tnn.BatchNorm2d(cout, eps=eps, momentum=momentum)]
    if act:
        layers.append(tnn.SiLU(inplace=True))
    return tnn.Sequential(*layers)


class SqueezeExcitation(tnn.Module):
    """torchvision's block: avgpool -> fc1 -> SiLU -> fc2 -> Sigmoid, multiplied onto the input.
    ``forward`` is the plain-torch NCHW form; the NHWC execution is in ``MBConv.run``."""

    def __init__(self, input_channels: int, squeeze_channels: int):
        super().__init__()
        self.avgpool = tnn.AdaptiveAvgPool2d(1)
        self.fc1 = mnn.XConv2d(input_channels, squeeze_channels, 1)
        self.fc2 = mnn.XConv2d(squeeze_channels, input_channels, 1)
        self.activation = tnn.SiLU(inplace=True)
        self.scale_activation = tnn.Sigmoid()

    def forward(self, x):
        s = F.adaptive_avg_pool2d(x, 1)
        return torch.sigmoid(self.fc2(F.silu(self.fc1(s)))) * x

    def gate(self, pm: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The pre-sigmoid gate [N, 1, 1, C] from the pooled map ``pm`` [N, C].  The squeeze width
        (4, 6, 10 ...) is no multiple of 8: both FCs take the odd-channel direct kernels, and the
        SiLU between them is a torch op on an [N, squeeze] tensor."""
        N, C = pm.shape
        return self.fc2.run(F.silu(self.fc1.run(pm.to(dtype).reshape(N, 1, 1, C))))


class MBConv(tnn.Module):
    def __init__(self, cin: int, cout: int, kernel: int, stride: int, expand_ratio: float,
                 sd_prob: float, eps: float, momentum: float):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError(f"stride must be 1 or 2, got {stride}")
        self.use_res_connect = stride == 1 and cin == cout
        expanded = _make_divisible(cin * expand_ratio, 8)
        self.expand = expanded != cin
        layers: List[tnn.Module] = []
        if self.expand:
            layers.append(_conv_bn_act(cin, expanded, 1, 1, 1, eps, momentum))
        layers.append(_conv_bn_act(expanded, expanded, kernel, stride, expanded, eps, momentum))
        layers.append(SqueezeExcitation(expanded, max(1, cin // 4)))
        layers.append(_conv_bn_act(expanded, cout, 1, 1, 1, eps, momentum, act=False))
        self.block = tnn.Sequential(*layers)
        self.stochastic_depth = tnn.Identity()  # torchvision's StochasticDepth(p, "row"): no state
        self.sd_prob = float(sd_prob)
        self.out_channels = cout
        self._one: Optional[torch.Tensor] = None

    def forward(self, x, keep_scale: Optional[torch.Tensor] = None):
        """torchvision semantics on NCHW, plain torch; ``keep_scale`` [N]: keep / (1 - p)."""
        y = self.block(x)
        if not self.use_res_connect:
            return y
        if keep_scale is not None:
            y = y * keep_scale.to(y.dtype).reshape(-1, 1, 1, 1)
        return x + y

    def _ones(self, like: torch.Tensor) -> torch.Tensor:
        """scale_residual's ``gamma``: a constant one per channel, without a gradient."""
        dt = torch.float64 if like.dtype == torch.float64 else torch.float32
        if self._one is None or self._one.device != like.device or self._one.dtype != dt:
            self._one = torch.ones(self.out_channels, device=like.device, dtype=dt)
        return self._one

    def run(self, x, seed=0, drop: bool = False):
        """x NHWC -> the block's output; ``drop``: training with this block's stochastic depth."""
        mods = list(self.block)
        drop = drop and self.use_res_connect and self.sd_prob > 0.0
        h = x
        if self.expand:
            h = conv_bn(h, mods[0][0], mods[0][1], "silu")
        dw = mods[-3]
        # the block input feeds the depthwise conv itself (expand ratio 1): the residual's
        # gradient is added in that conv's data-grad kernel
        slot = MF.ResidualSlot() if drop and not self.expand and dwconvk_route(h, dw[0]) else None
        z, pm = dwconv_bn_act_pool(h, dw[0], dw[1], "silu", pool=True, res_give=slot)
        h = MF.se_scale(z, mods[-2].gate(pm, z.dtype), "sigmoid")
        proj = mods[-1]
        if not drop:
            return conv_bn(h, proj[0], proj[1], "none",
                           residual=x if self.use_res_connect else None)
        f = conv_bn(h, proj[0], proj[1], "none")
        return MF.scale_residual(f, x, self._ones(f), self.sd_prob, seed, True, res_give=slot)

    def extra_repr(self) -> str:
        return f"stochastic_depth_prob={self.sd_prob:.4f}"


class EfficientNet(ZooModel):
    """``forward(x)``: x [B, 3, H, W] -> logits on mipipe's kernels; ``reference_forward(x)``: the
    same parameters (and, in training, the same keep masks) through plain torch."""

    def __init__(self, width_mult: float = 1.0, depth_mult: float = 1.0, dropout: float = 0.2,
                 stochastic_depth_prob: Optional[float] = 0.2, num_classes: int = 1000,
                 norm_eps: float = 1e-5, norm_momentum: float = 0.1,
                 compute_dtype: Optional[torch.dtype] = None, seed: int = 0, **_):
        super().__init__()
        if stochastic_depth_prob is None:
            stochastic_depth_prob = 0.2
        if not 0.0 <= stochastic_depth_prob < 1.0:
            raise ValueError(f"EfficientNet: stochastic_depth_prob must be in [0, 1), got "
                             f"{stochastic_depth_prob}")
        self.stochastic_depth_prob = float(stochastic_depth_prob)
        self.compute_dtype = compute_dtype
        self.seed = int(seed)
        self.rank_override: Optional[int] = None  # stochastic-depth seed rank
        self._sd_step = 0
        self._step_dev: Optional[torch.Tensor] = None  # device step counter (stochastic depth)
        self._last_seeds: Optional[List] = None

        def adj(c: int) -> int:
            return _make_divisible(c * width_mult, 8)

        depths = [int(math.ceil(n * depth_mult)) for *_r, n in _STAGES]
        total, done = sum(depths), 0
        eps, mom = norm_eps, norm_momentum
        features: List[tnn.Module] = [_conv_bn_act(3, adj(_STAGES[0][3]), 3, 2, 1, eps, mom)]
        for (ratio, kernel, stride, cin, cout, _n), depth in zip(_STAGES, depths):
            stage = []
            for i in range(depth):
                stage.append(MBConv(adj(cout if i else cin), adj(cout), kernel, 1 if i else stride,
                                    ratio, stochastic_depth_prob * done / total, eps, mom))
                done += 1
            features.append(tnn.Sequential(*stage))
        last_in = adj(_STAGES[-1][4])
        features.append(_conv_bn_act(last_in, 4 * last_in, 1, 1, 1, eps, mom))
        self.features = tnn.Sequential(*features)
        self.avgpool = tnn.AdaptiveAvgPool2d(1)
        self.classifier = tnn.Sequential(tnn.Dropout(p=dropout, inplace=True),
                                         mnn.Linear(4 * last_in, num_classes))
        for m in self.modules():
            if isinstance(m, tnn.Conv2d):
                tnn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    tnn.init.zeros_(m.bias)
            elif isinstance(m, tnn.BatchNorm2d):
                tnn.init.ones_(m.weight)
                tnn.init.zeros_(m.bias)
            elif isinstance(m, tnn.Linear):
                r = 1.0 / math.sqrt(m.out_features)
                tnn.init.uniform_(m.weight, -r, r)
                tnn.init.zeros_(m.bias)

    def blocks(self) -> List[MBConv]:
        return [b for stage in list(self.features)[1:-1] for b in stage]

    # ---- stochastic-depth seeds (as mipipe.models.convnext) ------------------------------------
    def _path_seeds(self, x: torch.Tensor, advance: bool) -> List:
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        if self.rank_override is not None:
            rank = self.rank_override
        base = (self.seed + 7919 * rank) & 0xFFFFFFFF
        n = len(self.blocks())
        if advance:
            self._sd_step += 1
        if advance and x.is_cuda:
            if self._step_dev is None or self._step_dev.device != x.device:
                self._step_dev = torch.full((1,), self._sd_step - 1, dtype=torch.int32,
                                            device=x.device)
            self._step_dev.add_(1)
            sdev = self._step_dev.clone()
            return [K.DevSeed(_seed(base, 0, i), sdev) for i in range(n)]
        return [_seed(base, self._sd_step, i) for i in range(n)]

    def run_model(self, x, ex):
        drop = self.training and self.stochastic_depth_prob > 0.0
        blocks = self.blocks()
        seeds = self._path_seeds(x, advance=True) if drop else [0] * len(blocks)
        if drop:
            self._last_seeds = seeds
        feats = list(self.features)
        x = run_seq(feats[0], x, ex)
        for blk, seed in zip(blocks, seeds):
            x = blk.run(x, seed, drop)
        x = run_seq(feats[-1], x, ex)
        return run_seq(self.classifier, global_pool(x), ex)

    def reference_forward(self, x):
        """Plain torch on NCHW; in training with stochastic depth it applies the keep masks of the
        last training ``forward`` (of the current step when there has been none)."""
        drop = self.training and self.stochastic_depth_prob > 0.0
        seeds = (self._last_seeds or self._path_seeds(x, advance=False)) if drop else None
        feats = list(self.features)
        x = feats[0](x.to(feats[0][0].weight.dtype))
        for i, blk in enumerate(self.blocks()):
            scale = None
            if drop and blk.use_res_connect and blk.sd_prob > 0.0:
                keep = K.drop_path_keep(x.shape[0], blk.sd_prob, seeds[i], x.device)
                inv = torch.tensor(1.0 / (1.0 - blk.sd_prob), dtype=torch.float32)
                scale = keep.to(x.dtype) * inv.to(x.dtype).to(x.device)
            x = blk(x, scale)
        x = feats[-1](x)
        x = F.adaptive_avg_pool2d(x, (1, 1)).reshape(x.shape[0], -1)
        return ref_linear(self.classifier[1], self.classifier[0](x))


def _factory(i: int):
    width, depth, dropout = _VARIANTS[i]

    def make(**kw) -> EfficientNet:
        kw.pop("pretrained", None)  # no network: pretrained weights cannot be fetched
        kw.setdefault("width_mult", width)
        kw.setdefault("depth_mult", depth)
        kw.setdefault("dropout", dropout)
        if i >= 5:  # torchvision builds b5 - b7 with BatchNorm2d(eps=1e-3, momentum=0.01)
            kw.setdefault("norm_eps", 1e-3)
            kw.setdefault("norm_momentum", 0.01)
        return EfficientNet(**kw)
    make.__name__ = f"efficientnet_b{i}"
    return make


for _i in range(8):
    _fn = _factory(_i)
    globals()[_fn.__name__] = _fn
    register_model(_fn.__name__, _fn)
