"""RegNet X / Y, 400MF ... 128GF (torchvision layout) on mipipe's NHWC kernels.

A block is a 1x1 convolution, a grouped 3x3 (stride 2 in a stage's first block) with a fixed
group width, in the Y models squeeze-excitation, and a 1x1 projection whose BatchNorm takes the
residual.  The stem and the 1x1 convolutions run on the MFMA implicit-GEMM conv with BatchNorm
statistics in its epilogue.  The grouped 3x3 (``f.b``) runs on ``gconv3.hip``'s MFMA kernels for
group widths 8 ... 64 (:func:`mipipe.models._zoo.gconv_bn_act_pool`: statistics from the conv's
own pass, BatchNorm + ReLU and the SE squeeze in ``bn_act_pool``); the models with wider groups
(y_16gf, y_32gf, y_128gf, x_8gf, x_16gf, x_32gf) and fp32 compute keep ``XConv2d.run``'s route for
it.  The SE gate is two 1x1 convolutions on the pooled ``[N, 1, 1, C]`` tensor and
``se_scale(..., "sigmoid")``.  ``state_dict`` keys and shapes follow torchvision
(``trunk_output.block1.block1-0.f.b.0.weight``, ``fc.weight`` ...).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import functional as MF

from . import register_model
from ._zoo import ZooModel, conv_bn, gconv_bn_act_pool, global_pool, ref_linear, run_seq
from .mobilenet import _make_divisible

__all__ = ["RegNet", "ResBottleneckBlock", "stage_params"]

#: name -> (depth, w_0, w_a, w_m, group width); the Y models add squeeze-excitation (ratio 0.25)
_CONFIGS = {
    "y_400mf": (16, 48, 27.89, 2.09, 8), "y_800mf": (14, 56, 38.84, 2.4, 16),
    "y_1_6gf": (27, 48, 20.71, 2.65, 24), "y_3_2gf": (21, 80, 42.63, 2.66, 24),
    "y_8gf": (17, 192, 76.82, 2.19, 56), "y_16gf": (18, 200, 106.23, 2.48, 112),
    "y_32gf": (20, 232, 115.89, 2.53, 232), "y_128gf": (27, 456, 160.83, 2.52, 264),
    "x_400mf": (22, 24, 24.48, 2.54, 16), "x_800mf": (16, 56, 35.73, 2.28, 16),
    "x_1_6gf": (18, 80, 34.01, 2.25, 24), "x_3_2gf": (25, 88, 26.31, 2.25, 48),
    "x_8gf": (23, 80, 49.56, 2.88, 120), "x_16gf": (22, 216, 55.59, 2.1, 128),
    "x_32gf": (23, 320, 69.86, 2.0, 168),
}
#: test-size models for 32 x 32 inputs: (depths, widths, group widths)
_NANO = ((1, 2), (24, 48), (8, 24))


def stage_params(depth: int, w_0: int, w_a: float, w_m: float,
                 group_width: int) -> Tuple[List[int], List[int], List[int]]:
    """(depths, widths, group widths) per stage, torchvision's ``BlockParams.from_init_params``
    with a bottleneck multiplier of 1: u_j = w_0 + w_a j, quantised to w_0 w_m^k and to multiples
    of 8 (in fp32, rounding half to even, as torchvision computes it), run-length encoded; then
    g = min(group width, w) and w rounded to a multiple of g."""
    if w_a < 0 or w_0 <= 0 or w_m <= 1 or w_0 % 8 != 0:
        raise ValueError("stage_params: invalid RegNet settings")
    u = torch.arange(depth, device="cpu") * w_a + w_0  # (also under a meta-device context)
    k = torch.round(torch.log(u / w_0) / math.log(w_m))
    ws = (torch.round(torch.divide(w_0 * torch.pow(w_m, k), 8)) * 8).int().tolist()
    widths, depths = [], []
    for w in ws:
        if widths and widths[-1] == w:
            depths[-1] += 1
        else:
            widths.append(w)
            depths.append(1)
    groups = [min(group_width, w) for w in widths]
    widths = [_make_divisible(w, g) for w, g in zip(widths, groups)]
    return depths, widths, groups


def _conv_bn_act(cin: int, cout: int, kernel: int, stride: int, groups: int,
                 act: bool = True) -> tnn.Sequential:
    """torchvision's Conv2dNormActivation: conv (no bias), BatchNorm, ReLU."""
    layers: List[tnn.Module] = [
        mnn.XConv2d(cin, cout, kernel, stride, (kernel - 1) // 2, groups=groups, bias=False),
        tnn.BatchNorm2d(cout)]
    if act:
        layers.append(tnn.ReLU(inplace=True))
    return tnn.Sequential(*layers)


class SqueezeExcitation(tnn.Module):
    """torchvision's block: avgpool -> fc1 -> ReLU -> fc2 -> Sigmoid, multiplied onto the input.
    ``forward`` is the plain-torch NCHW form; the NHWC execution is in ``ResBottleneckBlock.run``."""

    def __init__(self, input_channels: int, squeeze_channels: int):
        super().__init__()
        self.avgpool = tnn.AdaptiveAvgPool2d(1)
        self.fc1 = mnn.XConv2d(input_channels, squeeze_channels, 1)
        self.fc2 = mnn.XConv2d(squeeze_channels, input_channels, 1)
        self.activation = tnn.ReLU()
        self.scale_activation = tnn.Sigmoid()

    def forward(self, x):
        s = F.adaptive_avg_pool2d(x, 1)
        return torch.sigmoid(self.fc2(F.relu(self.fc1(s)))) * x

    def gate(self, pm: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The pre-sigmoid gate [N, 1, 1, C] from the pooled map ``pm`` [N, C]."""
        N, C = pm.shape
        return self.fc2.run(self.fc1.run(pm.to(dtype).reshape(N, 1, 1, C), "relu"))


class ResBottleneckBlock(tnn.Module):
    """x + F(x) with F = 1x1, grouped 3x3 (stride), [SE], 1x1; a strided 1x1 projection of x where
    the shape changes."""

    def __init__(self, width_in: int, width_out: int, stride: int, group_width: int,
                 se_ratio: Optional[float]):
        super().__init__()
        self.proj = None
        if width_in != width_out or stride != 1:
            self.proj = _conv_bn_act(width_in, width_out, 1, stride, 1, act=False)
        f: "OrderedDict[str, tnn.Module]" = OrderedDict()
        f["a"] = _conv_bn_act(width_in, width_out, 1, 1, 1)
        f["b"] = _conv_bn_act(width_out, width_out, 3, stride, width_out // group_width)
        if se_ratio:
            f["se"] = SqueezeExcitation(width_out, int(round(se_ratio * width_in)))
        f["c"] = _conv_bn_act(width_out, width_out, 1, 1, 1, act=False)
        self.f = tnn.Sequential(f)
        self.activation = tnn.ReLU(inplace=True)

    def forward(self, x):
        """torchvision semantics on NCHW, plain torch."""
        res = x if self.proj is None else self.proj(x)
        return F.relu(res + self.f(x))

    def run(self, x, ex=None):
        """x NHWC -> the block's output on mipipe's kernels."""
        f = self.f
        h = conv_bn(x, f.a[0], f.a[1], "relu")
        se = getattr(f, "se", None)
        z, pm = gconv_bn_act_pool(h, f.b[0], f.b[1], "relu", pool=se is not None)
        if se is not None:
            z = MF.se_scale(z, se.gate(pm, z.dtype), "sigmoid")
        res = x if self.proj is None else conv_bn(x, self.proj[0], self.proj[1], "none")
        return conv_bn(z, f.c[0], f.c[1], "relu", residual=res)


class RegNet(ZooModel):
    """``forward(x)``: x [B, 3, H, W] -> logits on mipipe's kernels; ``reference_forward(x)``: the
    same parameters through plain torch."""

    def __init__(self, depths: Sequence[int], widths: Sequence[int], group_widths: Sequence[int],
                 se_ratio: Optional[float] = None, num_classes: int = 1000, stem_width: int = 32,
                 compute_dtype: Optional[torch.dtype] = None, **_):
        super().__init__()
        self.compute_dtype = compute_dtype
        self.stem = _conv_bn_act(3, stem_width, 3, 2, 1)
        stages: "OrderedDict[str, tnn.Module]" = OrderedDict()
        cur = stem_width
        for i, (d, w, g) in enumerate(zip(depths, widths, group_widths), start=1):
            blocks: "OrderedDict[str, tnn.Module]" = OrderedDict()
            for j in range(d):
                blocks[f"block{i}-{j}"] = ResBottleneckBlock(cur if j == 0 else w, w,
                                                             2 if j == 0 else 1, g, se_ratio)
            stages[f"block{i}"] = tnn.Sequential(blocks)
            cur = w
        self.trunk_output = tnn.Sequential(stages)
        self.avgpool = tnn.AdaptiveAvgPool2d((1, 1))
        self.fc = mnn.Linear(cur, num_classes)
        for m in self.modules():
            if isinstance(m, tnn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                tnn.init.normal_(m.weight, mean=0.0, std=math.sqrt(2.0 / fan_out))
            elif isinstance(m, tnn.BatchNorm2d):
                tnn.init.ones_(m.weight)
                tnn.init.zeros_(m.bias)
            elif isinstance(m, tnn.Linear):
                tnn.init.normal_(m.weight, mean=0.0, std=0.01)
                tnn.init.zeros_(m.bias)

    def blocks(self) -> List[ResBottleneckBlock]:
        return [b for stage in self.trunk_output for b in stage]

    def run_model(self, x, ex):
        x = run_seq(self.stem, x, ex)
        for blk in self.blocks():
            x = blk.run(x, ex)
        return self.fc(global_pool(x))

    def reference_forward(self, x):
        """Plain torch on NCHW."""
        x = self.stem(x.to(self.stem[0].weight.dtype))
        x = self.trunk_output(x)
        x = F.adaptive_avg_pool2d(x, (1, 1)).reshape(x.shape[0], -1)
        return ref_linear(self.fc, x)


def _factory(name: str):
    def make(**kw) -> RegNet:
        kw.pop("pretrained", None)  # no network: pretrained weights cannot be fetched
        if name.endswith("nano"):
            depths, widths, groups = _NANO
        else:
            depths, widths, groups = stage_params(*_CONFIGS[name])
        if name.startswith("y"):
            kw.setdefault("se_ratio", 0.25)
        return RegNet(depths, widths, groups, **kw)
    make.__name__ = f"regnet_{name}"
    return make


for _n in list(_CONFIGS) + ["x_nano", "y_nano"]:
    _fn = _factory(_n)
    globals()[_fn.__name__] = _fn
    __all__.append(_fn.__name__)
    register_model(_fn.__name__, _fn)
