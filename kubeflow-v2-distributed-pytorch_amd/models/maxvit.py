"""MaxViT (torchvision's ``maxvit_t``) on mipipe's NHWC kernels.

The module tree and ``state_dict`` keys are torchvision's: ``stem.{0.0, 0.1, 1.0}``,
``blocks.i.layers.j.layers.MBconv.{proj.1, layers.{pre_norm, conv_a, conv_b, squeeze_excitation,
conv_c}}``, ``blocks.i.layers.j.layers.{window,grid}_attention.{attn_layer.{0, 1.to_qkv, 1.merge,
1.relative_position_bias_table, 1.relative_position_index}, mlp_layer.{0, 1, 3}}`` and
``classifier.{2, 3, 5}``.  ``relative_position_index`` is a buffer for key parity only: the
attention kernels compute the index.

Execution (``forward``): activations stay NHWC from the stem to the global pool, so an MBConv
output IS the token matrix [B*Hs*Ws, C] of the two attention layers that follow: no permutes.

* MBConv: BatchNorm (``pre_norm``), the MFMA 1x1 expansion with the BatchNorm statistics in its
  epilogue, ``dwconvk.hip``'s depthwise 3x3 (stride 1 / 2) with the statistics in the same pass,
  BatchNorm + exact GELU through ``se.hip``'s ``bn_act_pool(..., "gelu")`` (the second one with the
  squeeze-excitation block's pool), ``se_scale(..., "sigmoid")``, the 1x1 projection with bias; the
  shortcut is AvgPool2d(3, 2, 1) + 1x1 conv at stride 2; ``proj(x) + sd(layers(x))`` is
  :func:`MF.scale_residual` with a unit scale.
* window / grid attention: LayerNorm, the packed QKV GEMM, :func:`MF.partition_attention`
  (``relattn.hip``: 7x7 blocks or the dilated grid partition as address arithmetic, score scale
  C^-1/2 of the WHOLE width as torchvision defines it), the merge GEMM, then LayerNorm, the
  GELU-epilogue GEMM and the second GEMM; both residual adds are :func:`MF.scale_residual`.
* classifier: global average pool, LayerNorm, Linear, Tanh, bias-free Linear.

Stochastic depth runs in "row" mode, ``linspace(0, P, layers)`` over the layers, the five residual
branches of a layer at its probability with masks of their own; seeds as
:mod:`mipipe.models.convnext`.  Every stage map must be a whole number of 7x7 partitions: the
image side is a multiple of 32 * 7 (``maxvit_t``), other sizes raise.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Sequence

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import _ref
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K

from . import register_model
from ._zoo import ZooModel, conv_bn_act_pool, dwconv_bn_act_pool
from .convnext import _seed

__all__ = ["MaxVit", "maxvit_t", "maxvit_nano"]

_PART = 7
_HEAD_DIM = 32
_BN = dict(eps=1e-3, momentum=0.01)


def _conv_bn_gelu(cin: int, cout: int, kernel: int, stride: int, groups: int) -> tnn.Sequential:
    """torchvision's Conv2dNormActivation: conv (no bias), BatchNorm, GELU."""
    return tnn.Sequential(
        mnn.XConv2d(cin, cout, kernel, stride, (kernel - 1) // 2, groups=groups, bias=False),
        tnn.BatchNorm2d(cout, **_BN), tnn.GELU())


def _unit(m: tnn.Module, like: torch.Tensor, C: int) -> torch.Tensor:
    """scale_residual's ``gamma``: a constant one per channel, without a gradient."""
    dt = torch.float64 if like.dtype == torch.float64 else torch.float32
    one = m.__dict__.get("_one")
    if one is None or one.device != like.device or one.dtype != dt:
        one = m.__dict__["_one"] = torch.ones(C, device=like.device, dtype=dt)
    return one


def _scaled(t: torch.Tensor, keep_scale: Optional[torch.Tensor]) -> torch.Tensor:
    if keep_scale is None:
        return t
    return t * keep_scale.to(t.dtype).reshape(-1, *([1] * (t.dim() - 1)))


class SqueezeExcitation(tnn.Module):
    """avgpool -> fc1 -> SiLU -> fc2 -> Sigmoid, multiplied onto the input (NCHW, plain torch)."""

    def __init__(self, channels: int, squeeze: int):
        super().__init__()
        self.avgpool = tnn.AdaptiveAvgPool2d(1)
        self.fc1 = mnn.XConv2d(channels, squeeze, 1)
        self.fc2 = mnn.XConv2d(squeeze, channels, 1)
        self.activation = tnn.SiLU()
        self.scale_activation = tnn.Sigmoid()

    def forward(self, x):
        return torch.sigmoid(self.fc2(F.silu(self.fc1(F.adaptive_avg_pool2d(x, 1))))) * x

    def gate(self, pm: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The pre-sigmoid gate [N, 1, 1, C] from the pooled map ``pm`` [N, C]."""
        N, C = pm.shape
        return self.fc2.run(F.silu(self.fc1.run(pm.to(dtype).reshape(N, 1, 1, C))))


class MBConv(tnn.Module):
    def __init__(self, cin: int, cout: int, stride: int, sd_prob: float,
                 expansion: float = 4.0, squeeze: float = 0.25):
        super().__init__()
        proj: List[tnn.Module] = []
        if stride != 1 or cin != cout:
            proj = [mnn.XConv2d(cin, cout, 1, bias=True)]
            if stride == 2:
                proj = [tnn.AvgPool2d(3, stride=2, padding=1)] + proj
        self.proj = tnn.Sequential(*proj) if proj else tnn.Identity()
        mid = int(cout * expansion)
        self.stochastic_depth = tnn.Identity()  # StochasticDepth(p, "row"): no state
        self.layers = tnn.Sequential(OrderedDict(
            pre_norm=tnn.BatchNorm2d(cin, **_BN),
            conv_a=_conv_bn_gelu(cin, mid, 1, 1, 1),
            conv_b=_conv_bn_gelu(mid, mid, 3, stride, mid),
            squeeze_excitation=SqueezeExcitation(mid, int(cout * squeeze)),
            conv_c=mnn.XConv2d(mid, cout, 1, bias=True)))
        self.sd_prob, self.out_channels = float(sd_prob), cout

    def forward(self, x, keep_scale: Optional[torch.Tensor] = None):
        """torchvision semantics on NCHW, plain torch; ``keep_scale`` [N]: keep / (1 - p)."""
        return self.proj(x) + _scaled(self.layers(x), keep_scale)

    def run(self, x: torch.Tensor, seed, training: bool) -> torch.Tensor:
        """x NHWC -> the block's output."""
        L = self.layers
        res = x
        for m in (self.proj if isinstance(self.proj, tnn.Sequential) else ()):
            res = MF.avg_pool2d(res, 3, 2, 1) if isinstance(m, tnn.AvgPool2d) else m.run(res)
        h = MF.bn_act(x, L.pre_norm, "none")
        h = conv_bn_act_pool(h, L.conv_a[0], L.conv_a[1], "gelu")[0]
        z, pm = dwconv_bn_act_pool(h, L.conv_b[0], L.conv_b[1], "gelu", pool=True)
        h = MF.se_scale(z, L.squeeze_excitation.gate(pm, z.dtype), "sigmoid")
        f = L.conv_c.run(h)
        return MF.scale_residual(f, res, _unit(self, f, self.out_channels), self.sd_prob, seed,
                                 training)


class RelativePositionalMultiHeadAttention(tnn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.n_heads, self.head_dim = dim // _HEAD_DIM, _HEAD_DIM
        self.scale_factor = dim ** -0.5  # of the whole width: torchvision's definition
        self.to_qkv = mnn.Linear(dim, 3 * dim)
        self.merge = mnn.Linear(dim, dim)
        self.relative_position_bias_table = tnn.Parameter(
            torch.empty((2 * _PART - 1) ** 2, self.n_heads))
        self.register_buffer("relative_position_index", _ref.window_geometry(_PART, _PART, 0)[1])
        tnn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """torchvision's forward on partitions x [B, G, 49, C], plain torch."""
        B, G, P, C = x.shape
        H, DH = self.n_heads, self.head_dim
        q, k, v = torch.chunk(F.linear(x, self.to_qkv.weight, self.to_qkv.bias), 3, dim=-1)
        q, k, v = (t.reshape(B, G, P, H, DH).permute(0, 1, 3, 2, 4) for t in (q, k, v))
        dot = torch.einsum("bghid,bghjd->bghij", q, k * self.scale_factor)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)]
        p = F.softmax(dot + bias.view(P, P, -1).permute(2, 0, 1).unsqueeze(0), dim=-1)
        out = torch.einsum("bghij,bghjd->bghid", p, v).permute(0, 1, 3, 2, 4).reshape(B, G, P, C)
        return F.linear(out, self.merge.weight, self.merge.bias)


class PartitionAttentionLayer(tnn.Module):
    def __init__(self, dim: int, partition_type: str, sd_prob: float, mlp_ratio: int = 4):
        super().__init__()
        self.partition_type = partition_type
        self.mode = "block" if partition_type == "window" else "grid"
        self.attn_layer = tnn.Sequential(
            mnn.LayerNorm(dim), RelativePositionalMultiHeadAttention(dim), tnn.Dropout(0.0))
        self.mlp_layer = tnn.Sequential(
            mnn.LayerNorm(dim), mnn.Linear(dim, dim * mlp_ratio), tnn.GELU(),
            mnn.Linear(dim * mlp_ratio, dim), tnn.Dropout(0.0))
        self.stochastic_dropout = tnn.Identity()  # StochasticDepth(p, "row"): no state
        self.sd_prob, self.dim = float(sd_prob), dim

    def forward(self, x, keep_scales: Sequence[Optional[torch.Tensor]] = (None, None)):
        """torchvision semantics on NCHW, plain torch: partition, (swap), the two pre-LN residual
        branches, (swap), departition."""
        B, C, H, W = x.shape
        p = _PART if self.mode == "block" else H // _PART
        t = x.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1)
        t = t.reshape(B, (H // p) * (W // p), p * p, C)
        if self.mode == "grid":
            t = t.swapaxes(-2, -3)
        ln, at = self.attn_layer[0], self.attn_layer[1]
        t = t + _scaled(at(F.layer_norm(t, (C,), ln.weight, ln.bias, ln.eps)), keep_scales[0])
        ln, f1, f2 = self.mlp_layer[0], self.mlp_layer[1], self.mlp_layer[3]
        y = F.gelu(F.linear(F.layer_norm(t, (C,), ln.weight, ln.bias, ln.eps), f1.weight, f1.bias))
        t = t + _scaled(F.linear(y, f2.weight, f2.bias), keep_scales[1])
        if self.mode == "grid":
            t = t.swapaxes(-2, -3)
        t = t.reshape(B, H // p, W // p, p, p, C).permute(0, 5, 1, 3, 2, 4)
        return t.reshape(B, C, H, W)

    def _add(self, f, x, B, seed, training, slot):
        C = self.dim
        out = MF.scale_residual(f.reshape(B, -1, C), x.reshape(B, -1, C), _unit(self, f, C),
                                self.sd_prob, seed, training, bias_slot=slot)
        return out.reshape(-1, C)

    def run(self, x: torch.Tensor, B: int, Hs: int, Ws: int, seeds, training: bool):
        """x [B*Hs*Ws, C] (NHWC token rows) -> the layer's output rows."""
        at = self.attn_layer[1]
        s_a, s_f = MF.BiasGradSlot(), MF.BiasGradSlot()
        a = MF.partition_attention(at.to_qkv(self.attn_layer[0](x)),
                                   at.relative_position_bias_table, B, Hs, Ws, at.n_heads,
                                   self.mode, at.scale_factor)
        x = self._add(at.merge(a, bias_slot=s_a), x, B, seeds[0], training, s_a)
        f = self.mlp_layer[3](self.mlp_layer[1](self.mlp_layer[0](x), act="gelu"), bias_slot=s_f)
        return self._add(f, x, B, seeds[1], training, s_f)


class MaxVitLayer(tnn.Module):
    def __init__(self, cin: int, cout: int, stride: int, sd_prob: float):
        super().__init__()
        self.layers = tnn.Sequential(OrderedDict(
            MBconv=MBConv(cin, cout, stride, sd_prob),
            window_attention=PartitionAttentionLayer(cout, "window", sd_prob),
            grid_attention=PartitionAttentionLayer(cout, "grid", sd_prob)))
        self.sd_prob = float(sd_prob)


class MaxVitBlock(tnn.Module):
    def __init__(self, cin: int, cout: int, sd_probs: Sequence[float]):
        super().__init__()
        self.layers = tnn.ModuleList(
            MaxVitLayer(cout if i else cin, cout, 1 if i else 2, p) for i, p in enumerate(sd_probs))


class MaxVit(ZooModel):
    """``forward(x)``: x [B, 3, H, W] -> logits on mipipe's kernels; ``reference_forward(x)``: the
    same parameters (and, in training, the same keep masks) through plain torch on NCHW."""

    SITES = 5  # stochastic-depth sites of a layer: MBConv, 2 x window attention, 2 x grid attention

    def __init__(self, stem_channels: int = 64, block_channels: Sequence[int] = (64, 128, 256, 512),
                 block_layers: Sequence[int] = (2, 2, 5, 2),
                 stochastic_depth_prob: Optional[float] = 0.2, num_classes: int = 1000,
                 compute_dtype: Optional[torch.dtype] = None, seed: int = 0, **_):
        super().__init__()
        if stochastic_depth_prob is None:
            stochastic_depth_prob = 0.2
        if not 0.0 <= stochastic_depth_prob < 1.0:
            raise ValueError(f"MaxVit: stochastic_depth_prob must be in [0, 1), got "
                             f"{stochastic_depth_prob}")
        if any(c % _HEAD_DIM for c in block_channels):
            raise ValueError(f"MaxVit: every block width must be a multiple of {_HEAD_DIM} (the "
                             f"attention kernel's head width), got {tuple(block_channels)}")
        self.stochastic_depth_prob = float(stochastic_depth_prob)
        self.compute_dtype = compute_dtype
        self.seed = int(seed)
        self.rank_override: Optional[int] = None  # stochastic-depth seed rank
        self._sd_step = 0
        self._step_dev: Optional[torch.Tensor] = None  # device step counter (stochastic depth)
        self._last_seeds: Optional[List] = None
        self.stem = tnn.Sequential(
            _conv_bn_gelu(3, stem_channels, 3, 2, 1),
            tnn.Sequential(mnn.XConv2d(stem_channels, stem_channels, 3, 1, 1, bias=True)))
        n = sum(block_layers)
        probs = [stochastic_depth_prob * i / (n - 1) if n > 1 else 0.0 for i in range(n)]
        self.blocks = tnn.ModuleList()
        cin, at = stem_channels, 0
        for cout, depth in zip(block_channels, block_layers):
            self.blocks.append(MaxVitBlock(cin, cout, probs[at:at + depth]))
            cin, at = cout, at + depth
        self.classifier = tnn.Sequential(
            tnn.AdaptiveAvgPool2d(1), tnn.Flatten(), mnn.LayerNorm(cin), mnn.Linear(cin, cin),
            tnn.Tanh(), mnn.Linear(cin, num_classes, bias=False))
        for m in self.modules():
            if isinstance(m, (tnn.Conv2d, tnn.Linear)):
                tnn.init.normal_(m.weight, std=0.02)
                if m.bias is not None:
                    tnn.init.zeros_(m.bias)
            elif isinstance(m, tnn.BatchNorm2d):
                tnn.init.ones_(m.weight)
                tnn.init.zeros_(m.bias)

    def layers(self) -> List[MaxVitLayer]:
        return [layer for b in self.blocks for layer in b.layers]

    def _check_input(self, x: torch.Tensor):
        unit = 2 ** (1 + len(self.blocks)) * _PART
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[2] % unit:
            raise ValueError(
                f"MaxVit: expected [B, 3, S, S] images with S a multiple of {unit} (every stage "
                f"map a whole number of {_PART}x{_PART} partitions; maps are not padded), got "
                f"{tuple(x.shape)}")

    def _path_seeds(self, x: torch.Tensor, advance: bool) -> List:
        """One seed per residual branch for this step; see
        :meth:`mipipe.models.convnext.ConvNeXt._path_seeds`."""
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        if self.rank_override is not None:
            rank = self.rank_override
        base = (self.seed + 7919 * rank) & 0xFFFFFFFF
        n = self.SITES * len(self.layers())
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

    def forward(self, x: torch.Tensor):
        self._check_input(x)
        if x.is_cuda and self.activation_dtype(x) != torch.bfloat16:
            raise ValueError(f"MaxVit: compute dtype {self.activation_dtype(x)} on the GPU is not "
                             "supported — the LayerNorm and partition-attention kernels are bf16")
        return super().forward(x)

    def run_model(self, x, ex):
        training = self.training and self.stochastic_depth_prob > 0.0
        n = self.SITES * len(self.layers())
        seeds = self._path_seeds(x, advance=True) if training else [0] * n
        if training:
            self._last_seeds = seeds
        x = conv_bn_act_pool(x, self.stem[0][0], self.stem[0][1], "gelu")[0]
        x = self.stem[1][0].run(x)
        for i, layer in enumerate(self.layers()):
            s = seeds[self.SITES * i:self.SITES * (i + 1)]
            L = layer.layers
            x = L.MBconv.run(x, s[0], training)
            B, Hs, Ws, C = x.shape
            t = L.window_attention.run(x.reshape(-1, C), B, Hs, Ws, s[1:3], training)
            x = L.grid_attention.run(t, B, Hs, Ws, s[3:5], training).reshape(B, Hs, Ws, C)
        c = self.classifier
        return c[5](torch.tanh(c[3](c[2](MF.global_avg_pool(x)))))

    def reference_forward(self, x):
        """Plain torch on NCHW; in training with stochastic depth it applies the keep masks of the
        last training ``forward`` (of the current step when there has been none)."""
        self._check_input(x)
        training = self.training and self.stochastic_depth_prob > 0.0
        seeds = (self._last_seeds or self._path_seeds(x, advance=False)) if training else None
        x = self.stem(x.to(self.stem[0][0].weight.dtype))
        B = x.shape[0]

        def ks(p, seed):
            if not training or p <= 0.0:
                return None
            keep = K.drop_path_keep(B, p, seed, x.device)
            inv = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
            return keep.to(x.dtype) * inv.to(x.dtype).to(x.device)

        for i, layer in enumerate(self.layers()):
            s = seeds[self.SITES * i:self.SITES * (i + 1)] if training else [0] * self.SITES
            L, p = layer.layers, layer.sd_prob
            x = L.MBconv(x, ks(p, s[0]))
            x = L.window_attention(x, (ks(p, s[1]), ks(p, s[2])))
            x = L.grid_attention(x, (ks(p, s[3]), ks(p, s[4])))
        c = self.classifier
        y = F.layer_norm(x.mean((2, 3)), (x.shape[1],), c[2].weight, c[2].bias, c[2].eps)
        return F.linear(torch.tanh(F.linear(y, c[3].weight, c[3].bias)), c[5].weight)


def maxvit_t(**kw) -> MaxVit:
    kw.pop("pretrained", None)  # no network: pretrained weights cannot be fetched
    return MaxVit(64, (64, 128, 256, 512), (2, 2, 5, 2), **kw)


def maxvit_nano(**kw) -> MaxVit:
    """Stem 32, widths 32-64, layers 1-2: the variant the tests run, on 56 x 56 images (stage maps
    14 and 7: the grid partition strides are 2 and 1); no stochastic depth unless asked for."""
    kw.pop("pretrained", None)
    if kw.get("stochastic_depth_prob") is None:
        kw["stochastic_depth_prob"] = 0.0
    return MaxVit(32, (32, 64), (1, 2), **kw)


for _name, _fn in (("maxvit_t", maxvit_t), ("maxvit_nano", maxvit_nano)):
    register_model(_name, _fn)
