"""MobileNetV3 large / small (torchvision layout) on mipipe's NHWC kernels.

The inverted-residual blocks of MobileNetV2 with two additions: Hardswish on the ``HS`` rows and a
squeeze-excitation (SE) block after the depthwise convolution of the marked rows.  The 1x1
expansions / projections run on the MFMA implicit-GEMM conv with BatchNorm statistics in its
epilogue and the depthwise 3x3 / 5x5 on the vector direct kernels, as in MobileNetV2; BatchNorm +
Hardswish is ``se.hip``'s ``bn_act_pool`` (its backward recomputes the pre-activation, which
Hardswish's output does not determine), and in an SE block the same pass also produces the
squeeze, the two FCs run as 1x1 convolutions on the pooled ``[N, 1, 1, C]`` tensor, and
``se_scale`` multiplies the Hardsigmoid gate back.  ``state_dict`` keys and shapes follow
torchvision (``features.4.block.2.fc1.weight``, ``classifier.3.weight`` ...).
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import functional as MF

from . import register_model
from ._zoo import ZooModel, conv_bn, conv_bn_act_pool, global_pool, ref_linear, run_seq
from .mobilenet import _make_divisible

__all__ = ["MobileNetV3", "mobilenet_v3_large", "mobilenet_v3_small"]

_BN_EPS, _BN_MOMENTUM = 1e-3, 0.01


def _conv_bn_act(cin: int, cout: int, kernel_size: int = 1, stride: int = 1, groups: int = 1,
                 act: Optional[str] = None) -> tnn.Sequential:
    """torchvision's Conv2dNormActivation: conv (no bias), BatchNorm, activation."""
    layers: List[tnn.Module] = [
        mnn.XConv2d(cin, cout, kernel_size, stride, (kernel_size - 1) // 2, groups=groups,
                    bias=False),
        tnn.BatchNorm2d(cout, eps=_BN_EPS, momentum=_BN_MOMENTUM)]
    if act is not None:
        layers.append(tnn.Hardswish(inplace=True) if act == "HS" else tnn.ReLU(inplace=True))
    return tnn.Sequential(*layers)


class SqueezeExcitation(tnn.Module):
    """torchvision's block: avgpool -> fc1 -> ReLU -> fc2 -> Hardsigmoid, multiplied onto the input.
    ``forward`` is the plain-torch NCHW form; the NHWC execution is in ``InvertedResidual.run``,
    where the pool rides in the preceding BatchNorm pass."""

    def __init__(self, input_channels: int, squeeze_channels: int):
        super().__init__()
        self.avgpool = tnn.AdaptiveAvgPool2d(1)
        self.fc1 = mnn.XConv2d(input_channels, squeeze_channels, 1)
        self.fc2 = mnn.XConv2d(squeeze_channels, input_channels, 1)
        self.activation = tnn.ReLU()
        self.scale_activation = tnn.Hardsigmoid()

    def forward(self, x):
        s = F.adaptive_avg_pool2d(x, 1)
        s = F.hardsigmoid(self.fc2(F.relu(self.fc1(s))))
        return s * x

    def gate(self, pm: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The pre-Hardsigmoid gate [N, 1, 1, C] from the pooled map ``pm`` [N, C]."""
        N, C = pm.shape
        return self.fc2.run(self.fc1.run(pm.to(dtype).reshape(N, 1, 1, C), "relu"), "none")


class InvertedResidual(tnn.Module):
    def __init__(self, cin: int, kernel: int, expanded: int, cout: int, use_se: bool, act: str,
                 stride: int):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError(f"stride must be 1 or 2, got {stride}")
        self.use_res_connect = stride == 1 and cin == cout
        self.act = "hardswish" if act == "HS" else "relu"
        self.expand, self.use_se = expanded != cin, use_se
        layers: List[tnn.Module] = []
        if self.expand:
            layers.append(_conv_bn_act(cin, expanded, 1, act=act))
        layers.append(_conv_bn_act(expanded, expanded, kernel, stride, groups=expanded, act=act))
        if use_se:
            layers.append(SqueezeExcitation(expanded, _make_divisible(expanded // 4, 8)))
        layers.append(_conv_bn_act(expanded, cout, 1, act=None))
        self.block = tnn.Sequential(*layers)
        self.out_channels = cout

    def forward(self, x):  # torchvision semantics: NCHW, plain torch
        return x + self.block(x) if self.use_res_connect else self.block(x)

    def run(self, x, ex):
        mods = list(self.block)
        h = x
        if self.expand:
            h = conv_bn(h, mods[0][0], mods[0][1], self.act)
        dw = mods[1 if self.expand else 0]
        if self.use_se:
            z, pm = conv_bn_act_pool(h, dw[0], dw[1], self.act, pool=True)
            h = MF.se_scale(z, mods[-2].gate(pm, z.dtype))
        else:
            h = conv_bn(h, dw[0], dw[1], self.act)
        return conv_bn(h, mods[-1][0], mods[-1][1], "none",
                       residual=x if self.use_res_connect else None)


def _settings(arch: str, reduced_tail: bool):
    r = 2 if reduced_tail else 1
    if arch == "mobilenet_v3_large":
        rows = [  # input, kernel, expanded, out, SE, activation, stride
            (16, 3, 16, 16, False, "RE", 1), (16, 3, 64, 24, False, "RE", 2),
            (24, 3, 72, 24, False, "RE", 1), (24, 5, 72, 40, True, "RE", 2),
            (40, 5, 120, 40, True, "RE", 1), (40, 5, 120, 40, True, "RE", 1),
            (40, 3, 240, 80, False, "HS", 2), (80, 3, 200, 80, False, "HS", 1),
            (80, 3, 184, 80, False, "HS", 1), (80, 3, 184, 80, False, "HS", 1),
            (80, 3, 480, 112, True, "HS", 1), (112, 3, 672, 112, True, "HS", 1),
            (112, 5, 672, 160 // r, True, "HS", 2),
            (160 // r, 5, 960 // r, 160 // r, True, "HS", 1),
            (160 // r, 5, 960 // r, 160 // r, True, "HS", 1)]
        return rows, 1280 // r
    if arch == "mobilenet_v3_small":
        rows = [
            (16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2),
            (24, 3, 88, 24, False, "RE", 1), (24, 5, 96, 40, True, "HS", 2),
            (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
            (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1),
            (48, 5, 288, 96 // r, True, "HS", 2),
            (96 // r, 5, 576 // r, 96 // r, True, "HS", 1),
            (96 // r, 5, 576 // r, 96 // r, True, "HS", 1)]
        return rows, 1024 // r
    raise ValueError(f"unsupported MobileNetV3 arch {arch!r}")


class MobileNetV3(ZooModel):
    def __init__(self, arch: str = "mobilenet_v3_large", num_classes: int = 1000,
                 width_mult: float = 1.0, reduced_tail: bool = False, dropout: float = 0.2,
                 dilated: bool = False, compute_dtype: Optional[torch.dtype] = None, **_):
        super().__init__()
        if dilated:
            raise NotImplementedError("MobileNetV3: the dilated variant is not supported")
        rows, last_channel = _settings(arch, reduced_tail)

        def adj(c: int) -> int:
            return _make_divisible(c * width_mult, 8)

        first = adj(rows[0][0])
        features: List[tnn.Module] = [_conv_bn_act(3, first, 3, stride=2, act="HS")]
        for cin, k, exp, cout, se, act, stride in rows:
            features.append(InvertedResidual(adj(cin), k, adj(exp), adj(cout), se, act, stride))
        last_in = adj(rows[-1][3])
        last_out = 6 * last_in
        features.append(_conv_bn_act(last_in, last_out, 1, act="HS"))
        self.features = tnn.Sequential(*features)
        self.avgpool = tnn.AdaptiveAvgPool2d(1)
        self.last_channel = adj(last_channel)
        self.classifier = tnn.Sequential(
            mnn.Linear(last_out, self.last_channel), tnn.Hardswish(inplace=True),
            tnn.Dropout(p=dropout, inplace=True), mnn.Linear(self.last_channel, num_classes))
        self.compute_dtype = compute_dtype
        for m in self.modules():
            if isinstance(m, tnn.Conv2d):
                tnn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    tnn.init.zeros_(m.bias)
            elif isinstance(m, tnn.BatchNorm2d):
                tnn.init.ones_(m.weight)
                tnn.init.zeros_(m.bias)
            elif isinstance(m, tnn.Linear):
                tnn.init.normal_(m.weight, 0, 0.01)
                tnn.init.zeros_(m.bias)

    def run_model(self, x, ex):
        x = run_seq(self.features, x, ex)
        return run_seq(self.classifier, global_pool(x), ex)

    def reference_forward(self, x):
        x = self.features(x)
        x = F.adaptive_avg_pool2d(x, (1, 1)).reshape(x.shape[0], -1)
        x = F.hardswish(ref_linear(self.classifier[0], x))
        return ref_linear(self.classifier[3], self.classifier[2](x))


def _factory(arch: str):
    def make(**kw) -> MobileNetV3:
        kw.pop("pretrained", None)  # no network: pretrained weights cannot be fetched
        return MobileNetV3(arch, **kw)
    make.__name__ = arch
    return make


mobilenet_v3_large = _factory("mobilenet_v3_large")
mobilenet_v3_small = _factory("mobilenet_v3_small")

register_model("mobilenet_v3_large", mobilenet_v3_large)
register_model("mobilenet_v3_small", mobilenet_v3_small)
