"""ConvNeXt (torchvision's ``convnext_tiny`` / ``convnext_small`` / ``convnext_base`` /
``convnext_large``) on mipipe's kernels.

The module tree and ``state_dict`` keys are torchvision's: ``features.0.{0,1}`` the stem conv and
its LayerNorm, ``features.{1,3,5,7}.N`` the stages' blocks with ``block.0`` (7x7 depthwise conv),
``block.2`` (LayerNorm), ``block.3`` / ``block.5`` (Linear) and ``layer_scale``,
``features.{2,4,6}.{0,1}`` the downsample LayerNorm and 2x2/2 conv, ``classifier.0`` (LayerNorm)
and ``classifier.2`` (Linear), so checkpoints interchange.

Execution (``forward``), every step a HIP kernel, activations NHWC:

* the stem is a 4x4 stride-4 convolution of the image, i.e. a GEMM with K = 48 behind a
  permutation: :func:`MF.patchify` (its 4-pixel path) writes the image as GEMM rows in the column
  order of ``weight.view(C, 48)``, so the parameter is the weight operand as it stands;
* a block is :func:`MF.dwconv7` (halo-resident depthwise kernel), the channel LayerNorm on NHWC
  rows (``layernorm_fwd`` with H = C), the GELU Linear and the plain Linear, and
  :func:`MF.scale_residual` for ``x + drop_path(layer_scale * f)``.  The residual's gradient is
  added inside the depthwise data-grad kernel (``ResidualSlot``) and the second Linear's bias
  gradient is summed by the ``scale_residual`` backward (``BiasGradSlot``);
* a downsample is the channel LayerNorm and a dense MFMA convolution (bias in its epilogue);
* the head is ``global_avg_pool`` + LayerNorm + Linear.

Stochastic depth runs in "row" mode with ``p_i = P * i / (n - 1)`` over the n blocks; the keep
mask of block i is the dropout hash of (seed of the site and step, sample index).  On the GPU the
per-step part of the seed is a device counter, as in :mod:`mipipe.models.bert`, so a captured step
draws a new mask on every replay.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K

from . import register_model

_EPS = 1e-6


def _seed(base: int, step: int, site: int) -> int:
    return (base * 0x9E3779B1 + step * 0x85EBCA77 + site * 0xC2B2AE35 + 0x165667B1) & 0xFFFFFFFF


class _StemConv(mnn.ShadowMixin, tnn.Module):
    """``features.0.0``: the state of ``nn.Conv2d(in, C, 4, stride=4)`` (weight kept
    NCHW-contiguous), executed as a Linear over 4x4 patch rows."""

    def __init__(self, in_chans: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels, self.patch = in_chans, out_channels, 4
        self.weight = tnn.Parameter(torch.empty(out_channels, in_chans, 4, 4))
        self.bias = tnn.Parameter(torch.zeros(out_channels))

    def operand_view(self, w: torch.Tensor) -> torch.Tensor:
        return w.reshape(w.shape[0], -1)  # [C, in*16], columns (c, u, v): a view

    def forward(self, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """x [B, in, H, W] -> [B*(H/4)*(W/4), C] in ``dtype`` (bias included)."""
        tok = MF.patchify(x, 4, dtype)
        return MF.linear(tok, self.weight, self.compute_weight(dtype), self.bias)

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, kernel_size=4, stride=4"


class _DwConv7(mnn.XConv2d):
    """``block.0``: ``nn.Conv2d(C, C, 7, padding=3, groups=C)``; ``forward`` stays torch's NCHW
    convolution (the oracle), :meth:`run7` runs the depthwise kernels on NHWC activations."""

    def __init__(self, dim: int):
        super().__init__(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True)

    def run7(self, x: torch.Tensor, res_give=None) -> torch.Tensor:
        return MF.dwconv7(x, self.weight, self.compute_weight(x.dtype), self.bias, res_give)


class CNBlock(tnn.Module):
    def __init__(self, dim: int, layer_scale: float, sd_prob: float):
        super().__init__()
        # torchvision's Sequential: conv, Permute, LayerNorm, Linear, GELU, Linear, Permute
        self.block = tnn.Sequential(_DwConv7(dim), tnn.Identity(), mnn.LayerNorm(dim, eps=_EPS),
                                    mnn.Linear(dim, 4 * dim), tnn.GELU(), mnn.Linear(4 * dim, dim),
                                    tnn.Identity())
        self.layer_scale = tnn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.sd_prob = float(sd_prob)

    def forward(self, x: torch.Tensor, seed, training: bool) -> torch.Tensor:
        """x NHWC -> x + drop_path(layer_scale * mlp(LN(dwconv(x))))."""
        b = self.block
        slot, s_b = MF.ResidualSlot(), MF.BiasGradSlot()
        y = b[0].run7(x, res_give=slot)
        y = b[2](y.reshape(-1, y.shape[-1]))
        f = b[5](b[3](y, act="gelu"), bias_slot=s_b)
        return MF.scale_residual(f.reshape(x.shape), x, self.layer_scale, self.sd_prob, seed,
                                 training, bias_slot=s_b, res_give=slot)

    def extra_repr(self) -> str:
        return f"stochastic_depth_prob={self.sd_prob:.4f}"


def _ln_nhwc(ln: mnn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
    """torchvision's LayerNorm2d on an NHWC activation: the channel LayerNorm on its rows."""
    return ln(x.reshape(-1, x.shape[-1])).reshape(x.shape)


class ConvNeXt(tnn.Module):
    """``forward(x)``: x [B, C, H, W] (NCHW, fp32 or bf16; H and W multiples of 4) -> logits
    [B, num_classes] on mipipe's kernels; ``reference_forward(x)``: the same parameters (and, in
    training, the same keep masks) through plain torch."""

    def __init__(self, depths: Sequence[int], dims: Sequence[int], num_classes: int = 1000,
                 stochastic_depth_prob: float = 0.0, in_chans: int = 3,
                 compute_dtype: Optional[torch.dtype] = None, seed: int = 0,
                 layer_scale: float = 1e-6):
        super().__init__()
        if len(depths) != 4 or len(dims) != 4:
            raise ValueError("ConvNeXt: four stages are expected")
        if any(d % 8 for d in dims) or max(dims) > 2048:
            raise ValueError(f"ConvNeXt: stage widths must be multiples of 8 up to 2048 (the "
                             f"depthwise kernel's channel vectors), got {tuple(dims)}")
        if not 0.0 <= stochastic_depth_prob < 1.0:
            raise ValueError(f"ConvNeXt: stochastic_depth_prob must be in [0, 1), got "
                             f"{stochastic_depth_prob}")
        self.depths, self.dims, self.in_chans = tuple(depths), tuple(dims), in_chans
        self.stochastic_depth_prob = float(stochastic_depth_prob)
        self.compute_dtype = compute_dtype
        self.seed = int(seed)
        self.rank_override: Optional[int] = None  # stochastic-depth seed rank
        self._step = 0
        self._step_dev: Optional[torch.Tensor] = None  # device step counter (stochastic depth)
        self._last_seeds: Optional[List] = None
        total, done = sum(depths), 0
        layers: List[tnn.Module] = [
            tnn.Sequential(_StemConv(in_chans, dims[0]), mnn.LayerNorm(dims[0], eps=_EPS))]
        for i, (n, dim) in enumerate(zip(depths, dims)):
            stage = []
            for _ in range(n):
                p = stochastic_depth_prob * done / (total - 1.0) if total > 1 else 0.0
                stage.append(CNBlock(dim, layer_scale, p))
                done += 1
            layers.append(tnn.Sequential(*stage))
            if i < 3:
                layers.append(tnn.Sequential(
                    mnn.LayerNorm(dim, eps=_EPS),
                    mnn.XConv2d(dim, dims[i + 1], kernel_size=2, stride=2)))
        self.features = tnn.Sequential(*layers)
        self.avgpool = tnn.AdaptiveAvgPool2d(1)
        self.classifier = tnn.Sequential(mnn.LayerNorm(dims[-1], eps=_EPS), tnn.Flatten(1),
                                         mnn.Linear(dims[-1], num_classes))
        self._init_weights()

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, (tnn.Conv2d, tnn.Linear, _StemConv)):
                tnn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    tnn.init.zeros_(m.bias)

    def blocks(self) -> List[CNBlock]:
        return [b for i in (1, 3, 5, 7) for b in self.features[i]]

    def activation_dtype(self, x: torch.Tensor) -> torch.dtype:
        if self.compute_dtype is not None:
            return self.compute_dtype
        return torch.bfloat16 if x.is_cuda else torch.float32

    def _check_input(self, x: torch.Tensor):
        if x.dim() != 4 or x.shape[1] != self.in_chans:
            raise ValueError(f"ConvNeXt: expected [B, {self.in_chans}, H, W] input, got "
                             f"{tuple(x.shape)}")
        H, W = x.shape[2], x.shape[3]
        if H % 4 or W % 4 or H < 32 or W < 32:
            raise ValueError(f"ConvNeXt: image {H}x{W}: H and W must be multiples of 4 (the "
                             "stem's patch) and at least 32 (three 2x2/2 downsamples follow)")

    # ---- stochastic-depth seeds ---------------------------------------------------------------
    def _path_seeds(self, x: torch.Tensor, advance: bool) -> List:
        """One seed per block for this step.  ``advance``: a training forward (counts the step).
        On the GPU the per-step part is a device counter advanced by a device op and handed to
        the kernels as a snapshot (see :mod:`mipipe.models.bert`)."""
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        if self.rank_override is not None:
            rank = self.rank_override
        base = (self.seed + 7919 * rank) & 0xFFFFFFFF
        n = sum(self.depths)
        if advance:
            self._step += 1
        if advance and x.is_cuda:
            if self._step_dev is None or self._step_dev.device != x.device:
                self._step_dev = torch.full((1,), self._step - 1, dtype=torch.int32,
                                            device=x.device)
            self._step_dev.add_(1)
            sdev = self._step_dev.clone()
            return [K.DevSeed(_seed(base, 0, i), sdev) for i in range(n)]
        return [_seed(base, self._step, i) for i in range(n)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_input(x)
        dt = self.activation_dtype(x)
        if x.is_cuda and dt != torch.bfloat16:
            raise ValueError(
                f"ConvNeXt: compute dtype {dt} on the GPU is not supported — the LayerNorm "
                "kernels are bf16 (use compute_dtype=torch.bfloat16)")
        training = self.training and self.stochastic_depth_prob > 0.0
        seeds = self._path_seeds(x, advance=True) if training else [0] * sum(self.depths)
        if training:
            self._last_seeds = seeds
        B, H, W = x.shape[0], x.shape[2] // 4, x.shape[3] // 4
        stem = self.features[0]
        h = stem[1](stem[0](x, dt)).reshape(B, H, W, self.dims[0])
        site = 0
        for i in range(1, 8):
            if i % 2:
                for blk in self.features[i]:
                    h = blk(h, seeds[site], training)
                    site += 1
            else:
                ln, conv = self.features[i]
                h = conv.run(_ln_nhwc(ln, h))
        y = MF.global_avg_pool(h)
        return self.classifier[2](self.classifier[0](y))

    def reference_forward(self, x: torch.Tensor) -> torch.Tensor:
        """The same parameters through ``F.conv2d`` (``groups=C`` for the depthwise layers),
        ``F.layer_norm``, ``F.linear`` and exact GELU.  In training with stochastic depth it
        applies the keep masks of the last training ``forward`` (of the current step when there
        has been none), so both paths drop the same samples."""
        self._check_input(x)
        stem = self.features[0]
        w = stem[0].weight
        x = x.to(w.dtype)
        training = self.training and self.stochastic_depth_prob > 0.0
        seeds = None
        if training:
            seeds = self._last_seeds or self._path_seeds(x, advance=False)

        def ln2d(ln, t):
            return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), ln.weight, ln.bias,
                                _EPS).permute(0, 3, 1, 2)

        h = ln2d(stem[1], F.conv2d(x, w, stem[0].bias, stride=4))
        site = 0
        for i in range(1, 8):
            if i % 2:
                for blk in self.features[i]:
                    b = blk.block
                    y = F.conv2d(h, b[0].weight, b[0].bias, padding=3, groups=h.shape[1])
                    y = F.layer_norm(y.permute(0, 2, 3, 1), (h.shape[1],), b[2].weight, b[2].bias,
                                     _EPS)
                    y = F.linear(F.gelu(F.linear(y, b[3].weight, b[3].bias)), b[5].weight,
                                 b[5].bias)
                    y = blk.layer_scale * y.permute(0, 3, 1, 2)
                    if training and blk.sd_prob > 0.0:
                        keep = K.drop_path_keep(h.shape[0], blk.sd_prob, seeds[site], h.device)
                        inv = torch.tensor(1.0 / (1.0 - blk.sd_prob), dtype=torch.float32)
                        y = y * (keep.to(y.dtype) * inv.to(y.dtype).to(h.device)).reshape(-1, 1, 1, 1)
                    h = h + y
                    site += 1
            else:
                ln, conv = self.features[i]
                h = F.conv2d(ln2d(ln, h), conv.weight, conv.bias, stride=2)
        y = h.mean((2, 3))
        y = F.layer_norm(y, (y.shape[1],), self.classifier[0].weight, self.classifier[0].bias, _EPS)
        return F.linear(y, self.classifier[2].weight, self.classifier[2].bias)


def _convnext(depths, dims, default_sd: float, **kw) -> ConvNeXt:
    if kw.get("stochastic_depth_prob") is None:
        kw["stochastic_depth_prob"] = default_sd
    return ConvNeXt(depths, dims, **kw)


#: torchvision's stochastic-depth defaults
STOCHASTIC_DEPTH = {"convnext_tiny": 0.1, "convnext_small": 0.4, "convnext_base": 0.5,
                    "convnext_large": 0.5, "convnext_atto": 0.0}


def convnext_tiny(**kw) -> ConvNeXt:
    return _convnext((3, 3, 9, 3), (96, 192, 384, 768), 0.1, **kw)


def convnext_small(**kw) -> ConvNeXt:
    return _convnext((3, 3, 27, 3), (96, 192, 384, 768), 0.4, **kw)


def convnext_base(**kw) -> ConvNeXt:
    return _convnext((3, 3, 27, 3), (128, 256, 512, 1024), 0.5, **kw)


def convnext_large(**kw) -> ConvNeXt:
    return _convnext((3, 3, 27, 3), (192, 384, 768, 1536), 0.5, **kw)


def convnext_atto(**kw) -> ConvNeXt:
    """Depths 2-2-6-2, widths 40-80-160-320: the variant the tests run (no stochastic depth
    unless asked for)."""
    return _convnext((2, 2, 6, 2), (40, 80, 160, 320), 0.0, **kw)


for _name, _fn in (("convnext_tiny", convnext_tiny), ("convnext_small", convnext_small),
                   ("convnext_base", convnext_base), ("convnext_large", convnext_large),
                   ("convnext_atto", convnext_atto)):
    register_model(_name, _fn)
