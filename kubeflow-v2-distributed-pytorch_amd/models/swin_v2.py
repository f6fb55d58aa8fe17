"""Swin Transformer V2 (torchvision's ``swin_v2_t`` / ``swin_v2_s`` / ``swin_v2_b``) on mipipe's
kernels.

The module tree and ``state_dict`` keys are torchvision's, so checkpoints interchange: as
:mod:`mipipe.models.swin`, with ``attn.{qkv, proj, logit_scale [h, 1, 1], cpb_mlp.0 (Linear 2 ->
512), cpb_mlp.2 (Linear 512 -> h, no bias), relative_coords_table [1, 15, 15, 2],
relative_position_index}`` in a block and ``features.{2,4,6}.{reduction, norm}`` with the
LayerNorm over 2C after the reduction.

What differs from V1 in execution:

* 8x8 windows (shift 4), and cosine attention: :func:`MF.window_attention_v2` (winattn8.hip)
  normalises q and k per token and head in fp32 inside the kernel and multiplies the cosines by
  ``exp(min(logit_scale, ln 100))``;
* the position bias is ``16 * sigmoid(cpb_mlp(relative_coords_table))``, 225 rows, computed once
  per block and step in fp32 with plain torch ops; autograd carries the kernel's ``dbias`` back
  through the MLP;
* the key third of ``qkv.bias`` is held at zero: the forward multiplies the bias by a constant
  0 / 1 vector (the parameter's storage is not written), which also zeroes that third's gradient;
* post-norm blocks: ``x + sd(norm1(attn(x)))`` then ``x + sd(norm2(mlp(x)))`` — the LayerNorm
  kernels after ``proj`` / ``mlp.3`` (their backward also sums the producing Linear's bias
  gradient) and :func:`MF.scale_residual` with a unit scale for stochastic depth + residual add;
* a patch merging is ``norm(reduction(patch_merge(x)))``.

Stage maps must be whole numbers of 8x8 windows (and even before a merge): image sides are
multiples of 256 for t / s / b; other sizes raise, nothing is padded.
"""
from __future__ import annotations

import math

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import _ref
from mipipe.ops import functional as MF

from . import register_model
from .swin import _EPS, _ln, _shifts, PatchMerging, SwinBlock, SwinTransformer

_WIN = 8


def _coords_table() -> torch.Tensor:
    """[1, 15, 15, 2]: sign(x) * log2(|8x / 7| + 1) / 3 over the relative offsets -7..7."""
    r = torch.arange(-(_WIN - 1), _WIN, dtype=torch.float32)
    t = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1)[None] / (_WIN - 1) * 8
    return torch.sign(t) * torch.log2(t.abs() + 1.0) / 3.0


class ShiftedWindowAttentionV2(tnn.Module):
    window = _WIN

    def __init__(self, dim: int, heads: int, shift: int):
        super().__init__()
        self.num_heads, self.shift = heads, shift
        self.qkv = mnn.Linear(dim, 3 * dim)
        self.proj = mnn.Linear(dim, dim)
        self.logit_scale = tnn.Parameter(torch.full((heads, 1, 1), math.log(10.0)))
        self.cpb_mlp = tnn.Sequential(tnn.Linear(2, 512, bias=True), tnn.ReLU(inplace=True),
                                      tnn.Linear(512, heads, bias=False))
        self.register_buffer("relative_coords_table", _coords_table())
        self.register_buffer("relative_position_index",
                             _ref.window_geometry(_WIN, _WIN, 0, win=_WIN)[1].reshape(-1))
        # 1 on the q and v thirds of qkv.bias, 0 on the k third (not in state_dict)
        keep = torch.ones(3, dim)
        keep[1] = 0
        self.register_buffer("_keep_bias", keep.reshape(-1), persistent=False)

    def position_bias(self) -> torch.Tensor:
        """[225, heads]: 16 * sigmoid(cpb_mlp(coords)); indexed by relative_position_index."""
        return 16 * torch.sigmoid(self.cpb_mlp(self.relative_coords_table).view(-1, self.num_heads))

    def reference_qkv_bias(self) -> torch.Tensor:
        return self.qkv.bias * self._keep_bias

    def reference_scores(self, q: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
        N = q.shape[-2]
        a = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)
        a = a * torch.clamp(self.logit_scale, max=math.log(100.0)).exp()
        bias = self.position_bias()[self.relative_position_index]
        return a + bias.view(N, N, -1).permute(2, 0, 1)

    def forward(self, x: torch.Tensor, B: int, Hs: int, Ws: int, bias_slot=None) -> torch.Tensor:
        qkv = MF.linear(x, self.qkv.weight, self.qkv.compute_weight(x.dtype),
                        self.reference_qkv_bias())
        a = MF.window_attention_v2(qkv, self.position_bias(), self.logit_scale, B, Hs, Ws,
                                   self.num_heads, _shifts(Hs, Ws, self.shift, _WIN))
        return self.proj(a, bias_slot=bias_slot)


class SwinBlockV2(SwinBlock):
    attn_cls = ShiftedWindowAttentionV2

    def forward(self, x: torch.Tensor, B: int, Hs: int, Ws: int, seeds, training: bool):
        """x [B*Hs*Ws, C] -> the block's output rows (post-norm)."""
        s_a, s_f = MF.BiasGradSlot(), MF.BiasGradSlot()
        a = self.norm1(self.attn(x, B, Hs, Ws, bias_slot=s_a), bias_slot=s_a)
        x = self._add(a, x, B, seeds[0], training, None)
        f = self.mlp[3](self.mlp[0](x, act="gelu"), bias_slot=s_f)
        return self._add(self.norm2(f, bias_slot=s_f), x, B, seeds[1], training, None)


class PatchMergingV2(PatchMerging):
    def __init__(self, dim: int):
        super().__init__(dim)
        self.norm = mnn.LayerNorm(2 * dim, eps=_EPS)

    def forward(self, x: torch.Tensor, B: int, Hs: int, Ws: int) -> torch.Tensor:
        return self.norm(self.reduction(MF.patch_merge(x, B, Hs, Ws)))


class SwinTransformerV2(SwinTransformer):
    """:class:`mipipe.models.swin.SwinTransformer` with V2's blocks, mergings and 8x8 windows;
    ``reference_forward`` is torchvision's V2 composition (``F.normalize``, matmul, softmax, roll,
    partition) on the same parameters and keep masks."""
    window, block_cls, merge_cls = _WIN, SwinBlockV2, PatchMergingV2

    @staticmethod
    def _reference_merge(f, t):
        return _ln(f.norm, F.linear(t, f.reduction.weight))

    def _reference_block(self, blk, h, sd, s0, s1):
        h = h + sd(_ln(blk.norm1, self._reference_attention(blk.attn, h)), blk.sd_prob, s0)
        y = F.gelu(F.linear(h, blk.mlp[0].weight, blk.mlp[0].bias))
        y = F.linear(y, blk.mlp[3].weight, blk.mlp[3].bias)
        return h + sd(_ln(blk.norm2, y), blk.sd_prob, s1)


def _swin_v2(embed_dim, depths, heads, default_sd: float, **kw) -> SwinTransformerV2:
    if kw.get("stochastic_depth_prob") is None:
        kw["stochastic_depth_prob"] = default_sd
    return SwinTransformerV2(embed_dim, depths, heads, **kw)


def swin_v2_t(**kw) -> SwinTransformerV2:
    return _swin_v2(96, (2, 2, 6, 2), (3, 6, 12, 24), 0.2, **kw)


def swin_v2_s(**kw) -> SwinTransformerV2:
    return _swin_v2(96, (2, 2, 18, 2), (3, 6, 12, 24), 0.3, **kw)


def swin_v2_b(**kw) -> SwinTransformerV2:
    return _swin_v2(128, (2, 2, 18, 2), (4, 8, 16, 32), 0.5, **kw)


def swin_v2_nano(**kw) -> SwinTransformerV2:
    """Embed 32, depths 2-2-2, heads 1-2-4: the variant the tests run, on 128 x 128 images (stage
    maps 32, 16 and 8; no stochastic depth unless asked for)."""
    return _swin_v2(32, (2, 2, 2), (1, 2, 4), 0.0, **kw)


for _name, _fn in (("swin_v2_t", swin_v2_t), ("swin_v2_s", swin_v2_s), ("swin_v2_b", swin_v2_b),
                   ("swin_v2_nano", swin_v2_nano)):
    register_model(_name, _fn)
