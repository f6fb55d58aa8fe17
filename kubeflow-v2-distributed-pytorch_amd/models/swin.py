"""Swin Transformer (torchvision's ``swin_t`` / ``swin_s`` / ``swin_b``) on mipipe's kernels.

The module tree and ``state_dict`` keys are torchvision's: ``features.0.{0,2}`` the 4x4 stride-4
patch convolution and its LayerNorm, ``features.{1,3,5,7}.N`` the stages' blocks with ``norm1``,
``attn.{qkv, proj, relative_position_bias_table, relative_position_index}``, ``norm2``,
``mlp.{0,3}``, ``features.{2,4,6}.{reduction, norm}`` the patch mergings, ``norm`` and ``head``,
so checkpoints interchange.  ``relative_position_index`` is kept as a buffer for key parity only:
the attention kernels compute the index.

Execution (``forward``), every step a HIP kernel, activations as NHWC token rows [B*Hs*Ws, C]:

* the stem is :func:`MF.patchify` (its 4-pixel path) and a GEMM with K = 48 on
  ``weight.view(C, 48)``, as in ConvNeXt;
* a block is ``x + sd(proj(winattn(qkv(norm1 x))))`` then ``x + sd(mlp(norm2 x))``: the LayerNorm
  kernels, the packed QKV GEMM, :func:`MF.window_attention` (7x7 windows, head width 32; the
  cyclic shift of every second block, the window partition and their inverses are address
  arithmetic inside the kernel), the GELU-epilogue GEMM, and :func:`MF.scale_residual` with a
  constant unit scale for stochastic depth + residual add (it also sums the producing Linear's
  bias gradient);
* a patch merging is :func:`MF.patch_merge` (the 2x2 gather), the LayerNorm over 4C and the
  bias-free reduction GEMM;
* the head is ``norm``, the global average over tokens and ``head``.

Stochastic depth runs in "row" mode with ``p_i = P * i / (n - 1)`` over the n blocks, both
residual branches of block i at ``p_i`` with masks of their own; the seeds follow
:mod:`mipipe.models.convnext` (a device step counter on the GPU, so a captured step draws new
masks on every replay).  Stage maps must be whole numbers of 7x7 windows (and even before a
merge): other image sizes raise, nothing is padded.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import _ref
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K

from . import register_model
from .convnext import _StemConv, _seed

_EPS = 1e-5
_WIN = 7
_HEAD_DIM = 32  # the window-attention kernel's head width


def _shifts(Hs: int, Ws: int, shift: int, win: int = _WIN):
    """torchvision's rule: an axis the window covers whole is not shifted."""
    return (0 if Hs <= win else shift, 0 if Ws <= win else shift)


class ShiftedWindowAttention(tnn.Module):
    window = _WIN

    def __init__(self, dim: int, heads: int, shift: int):
        super().__init__()
        self.num_heads, self.shift = heads, shift
        self.qkv = mnn.Linear(dim, 3 * dim)
        self.proj = mnn.Linear(dim, dim)
        self.relative_position_bias_table = tnn.Parameter(
            torch.zeros((2 * _WIN - 1) ** 2, heads))
        self.register_buffer("relative_position_index",
                             _ref.window_geometry(_WIN, _WIN, 0)[1].reshape(-1))

    def forward(self, y: torch.Tensor, B: int, Hs: int, Ws: int, bias_slot=None) -> torch.Tensor:
        a = MF.window_attention(self.qkv(y), self.relative_position_bias_table, B, Hs, Ws,
                                self.num_heads, _shifts(Hs, Ws, self.shift))
        return self.proj(a, bias_slot=bias_slot)

    def reference_scores(self, q: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
        """q, k [B*nW, heads, N, D] -> the scores with the position bias, in plain torch ops."""
        N = q.shape[-2]
        a = (q * q.shape[-1] ** -0.5) @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index]
        return a + bias.view(N, N, -1).permute(2, 0, 1)

    def reference_qkv_bias(self) -> torch.Tensor:
        return self.qkv.bias


class _MLP(tnn.Sequential):
    """torchvision's ``MLP``: Linear, GELU, Dropout, Linear, Dropout (keys ``0`` and ``3``)."""

    def __init__(self, dim: int, hidden: int):
        super().__init__(mnn.Linear(dim, hidden), tnn.GELU(), tnn.Dropout(0.0),
                         mnn.Linear(hidden, dim), tnn.Dropout(0.0))


class SwinBlock(tnn.Module):
    attn_cls = ShiftedWindowAttention

    def __init__(self, dim: int, heads: int, shift: int, sd_prob: float):
        super().__init__()
        self.norm1 = mnn.LayerNorm(dim, eps=_EPS)
        self.attn = self.attn_cls(dim, heads, shift)
        self.norm2 = mnn.LayerNorm(dim, eps=_EPS)
        self.mlp = _MLP(dim, 4 * dim)
        self.sd_prob = float(sd_prob)
        # scale_residual's per-channel scale: a constant 1 (not a parameter, not in state_dict)
        self.register_buffer("_unit", torch.ones(dim), persistent=False)

    def _add(self, f, x, B, seed, training, slot):
        C = x.shape[-1]
        out = MF.scale_residual(f.reshape(B, -1, C), x.reshape(B, -1, C), self._unit, self.sd_prob,
                                seed, training, bias_slot=slot)
        return out.reshape(-1, C)

    def forward(self, x: torch.Tensor, B: int, Hs: int, Ws: int, seeds, training: bool):
        """x [B*Hs*Ws, C] -> the block's output rows."""
        s_a, s_f = MF.BiasGradSlot(), MF.BiasGradSlot()
        x = self._add(self.attn(self.norm1(x), B, Hs, Ws, bias_slot=s_a), x, B, seeds[0], training,
                      s_a)
        f = self.mlp[3](self.mlp[0](self.norm2(x), act="gelu"), bias_slot=s_f)
        return self._add(f, x, B, seeds[1], training, s_f)

    def extra_repr(self) -> str:
        return f"stochastic_depth_prob={self.sd_prob:.4f}"


class PatchMerging(tnn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.reduction = mnn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = mnn.LayerNorm(4 * dim, eps=_EPS)

    def forward(self, x: torch.Tensor, B: int, Hs: int, Ws: int) -> torch.Tensor:
        return self.reduction(self.norm(MF.patch_merge(x, B, Hs, Ws)))


def _ln(m, t):
    return F.layer_norm(t, (t.shape[-1],), m.weight, m.bias, _EPS)


class SwinTransformer(tnn.Module):
    """``forward(x)``: x [B, C, H, W] (NCHW, fp32 or bf16) -> logits [B, num_classes] on mipipe's
    kernels; ``reference_forward(x)``: the same parameters (and, in training, the same keep masks)
    through ``torch.roll``, an explicit window partition, ``F.softmax``, ``F.layer_norm`` and
    ``F.linear``."""
    window, block_cls, merge_cls = _WIN, SwinBlock, PatchMerging

    def __init__(self, embed_dim: int, depths: Sequence[int], num_heads: Sequence[int],
                 num_classes: int = 1000, stochastic_depth_prob: float = 0.0, in_chans: int = 3,
                 compute_dtype: Optional[torch.dtype] = None, seed: int = 0):
        super().__init__()
        dims = [embed_dim * 2 ** i for i in range(len(depths))]
        if len(depths) != len(num_heads) or any(d != h * _HEAD_DIM for d, h in zip(dims, num_heads)):
            raise ValueError(f"SwinTransformer: every stage needs width / heads == {_HEAD_DIM} "
                             f"(the window-attention kernel's head width), got widths {dims} and "
                             f"heads {tuple(num_heads)}")
        if max(dims) > 2048 or (len(dims) > 1 and 4 * dims[-2] > 2048):
            raise ValueError("SwinTransformer: a LayerNorm (4x the width at a patch merging) is "
                             "wider than the LayerNorm kernels' 2048")
        if not 0.0 <= stochastic_depth_prob < 1.0:
            raise ValueError(f"SwinTransformer: stochastic_depth_prob must be in [0, 1), got "
                             f"{stochastic_depth_prob}")
        self.depths, self.dims, self.num_heads = tuple(depths), tuple(dims), tuple(num_heads)
        self.in_chans = in_chans
        self.stochastic_depth_prob = float(stochastic_depth_prob)
        self.compute_dtype = compute_dtype
        self.seed = int(seed)
        self.rank_override: Optional[int] = None  # stochastic-depth seed rank
        self._step = 0
        self._step_dev: Optional[torch.Tensor] = None  # device step counter (stochastic depth)
        self._last_seeds: Optional[List] = None
        total, done = sum(depths), 0
        layers: List[tnn.Module] = [tnn.Sequential(
            _StemConv(in_chans, dims[0]), tnn.Identity(), mnn.LayerNorm(dims[0], eps=_EPS))]
        for i, (n, dim, heads) in enumerate(zip(depths, dims, num_heads)):
            stage = []
            for j in range(n):
                p = stochastic_depth_prob * done / (total - 1.0) if total > 1 else 0.0
                shift = 0 if j % 2 == 0 else self.window // 2
                stage.append(self.block_cls(dim, heads, shift, p))
                done += 1
            layers.append(tnn.Sequential(*stage))
            if i + 1 < len(depths):
                layers.append(self.merge_cls(dim))
        self.features = tnn.Sequential(*layers)
        self.norm = mnn.LayerNorm(dims[-1], eps=_EPS)
        self.head = mnn.Linear(dims[-1], num_classes)
        self._init_weights()

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, tnn.Linear):
                tnn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    tnn.init.zeros_(m.bias)
            elif isinstance(m, ShiftedWindowAttention):
                tnn.init.trunc_normal_(m.relative_position_bias_table, std=0.02)
        stem = self.features[0][0]  # nn.Conv2d's own initialisation, as torchvision leaves it
        tnn.init.kaiming_uniform_(stem.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(stem.in_channels * 16)
        tnn.init.uniform_(stem.bias, -bound, bound)

    def blocks(self) -> List[SwinBlock]:
        return [b for f in self.features if isinstance(f, tnn.Sequential) for b in f
                if isinstance(b, SwinBlock)]

    def activation_dtype(self, x: torch.Tensor) -> torch.dtype:
        if self.compute_dtype is not None:
            return self.compute_dtype
        return torch.bfloat16 if x.is_cuda else torch.float32

    def _check_input(self, x: torch.Tensor):
        if x.dim() != 4 or x.shape[1] != self.in_chans:
            raise ValueError(f"SwinTransformer: expected [B, {self.in_chans}, H, W] input, got "
                             f"{tuple(x.shape)}")
        H, W, n = x.shape[2], x.shape[3], len(self.depths)
        unit = 4 * self.window * 2 ** (n - 1)
        if H % unit or W % unit or H < unit or W < unit:
            raise ValueError(
                f"SwinTransformer: image {H}x{W}: every stage map must be a whole number of "
                f"{self.window}x{self.window} windows, so H and W must be multiples of {unit} "
                f"(4-pixel patches, {n - 1} patch mergings); maps are not padded")

    def _path_seeds(self, x: torch.Tensor, advance: bool) -> List:
        """One seed per residual branch (two per block) for this step; see
        :meth:`mipipe.models.convnext.ConvNeXt._path_seeds`."""
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
        if self.rank_override is not None:
            rank = self.rank_override
        base = (self.seed + 7919 * rank) & 0xFFFFFFFF
        n = 2 * sum(self.depths)
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
                f"SwinTransformer: compute dtype {dt} on the GPU is not supported — the "
                "LayerNorm and window-attention kernels are bf16 (use "
                "compute_dtype=torch.bfloat16)")
        training = self.training and self.stochastic_depth_prob > 0.0
        seeds = self._path_seeds(x, advance=True) if training else [0] * (2 * sum(self.depths))
        if training:
            self._last_seeds = seeds
        B, Hs, Ws = x.shape[0], x.shape[2] // 4, x.shape[3] // 4
        stem = self.features[0]
        h = stem[2](stem[0](x, dt))
        site = 0
        for f in list(self.features)[1:]:
            if isinstance(f, PatchMerging):
                h = f(h, B, Hs, Ws)
                Hs, Ws = Hs // 2, Ws // 2
                continue
            for blk in f:
                h = blk(h, B, Hs, Ws, seeds[site:site + 2], training)
                site += 2
        y = MF.global_avg_pool(self.norm(h).reshape(B, Hs, Ws, -1))
        return self.head(y)

    def reference_forward(self, x: torch.Tensor) -> torch.Tensor:
        """torchvision's composition on the same parameters.  In training with stochastic depth it
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
        B = x.shape[0]

        def sd(t, p, seed):
            if not training or p <= 0.0:
                return t
            keep = K.drop_path_keep(B, p, seed, t.device).to(t.dtype)
            inv = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).to(t.dtype).to(t.device)
            return t * (keep * inv).reshape(-1, 1, 1, 1)

        h = _ln(stem[2], F.conv2d(x, w, stem[0].bias, stride=4).permute(0, 2, 3, 1))
        site = 0
        for f in list(self.features)[1:]:
            if isinstance(f, PatchMerging):
                parts = [h[:, 0::2, 0::2], h[:, 1::2, 0::2], h[:, 0::2, 1::2], h[:, 1::2, 1::2]]
                h = self._reference_merge(f, torch.cat(parts, -1))
                continue
            for blk in f:
                s0, s1 = (seeds[site], seeds[site + 1]) if training else (0, 0)
                h = self._reference_block(blk, h, sd, s0, s1)
                site += 2
        y = _ln(self.norm, h).mean((1, 2))
        return F.linear(y, self.head.weight, self.head.bias)

    @staticmethod
    def _reference_merge(f, t):
        return F.linear(_ln(f.norm, t), f.reduction.weight)

    def _reference_block(self, blk, h, sd, s0, s1):
        h = h + sd(self._reference_attention(blk.attn, _ln(blk.norm1, h)), blk.sd_prob, s0)
        y = F.gelu(F.linear(_ln(blk.norm2, h), blk.mlp[0].weight, blk.mlp[0].bias))
        return h + sd(F.linear(y, blk.mlp[3].weight, blk.mlp[3].bias), blk.sd_prob, s1)

    @staticmethod
    def _reference_attention(at, t):
        B, H, W, C = t.shape
        win = at.window
        sy, sx = _shifts(H, W, at.shift, win)
        if sy or sx:
            t = torch.roll(t, (-sy, -sx), (1, 2))
        nW, N, nh = (H // win) * (W // win), win * win, at.num_heads
        t = t.view(B, H // win, win, W // win, win, C).permute(0, 1, 3, 2, 4, 5)
        qkv = F.linear(t.reshape(B * nW, N, C), at.qkv.weight, at.reference_qkv_bias())
        q, k, v = qkv.reshape(B * nW, N, 3, nh, C // nh).permute(2, 0, 3, 1, 4)
        a = at.reference_scores(q, k)
        if sy or sx:
            img = t.new_zeros(H, W)
            count = 0
            for hs in ((0, -win), (-win, -sy), (-sy, None)):
                for ws in ((0, -win), (-win, -sx), (-sx, None)):
                    img[hs[0]:hs[1], ws[0]:ws[1]] = count
                    count += 1
            img = img.view(H // win, win, W // win, win).permute(0, 2, 1, 3).reshape(nW, N)
            m = img[:, None, :] - img[:, :, None]
            m = m.masked_fill(m != 0, -100.0)
            a = (a.view(B, nW, nh, N, N) + m[None, :, None]).view(B * nW, nh, N, N)
        o = (F.softmax(a, -1) @ v).transpose(1, 2).reshape(B * nW, N, C)
        o = F.linear(o, at.proj.weight, at.proj.bias)
        o = o.view(B, H // win, W // win, win, win, C).permute(0, 1, 3, 2, 4, 5)
        o = o.reshape(B, H, W, C)
        return torch.roll(o, (sy, sx), (1, 2)) if sy or sx else o


def _swin(embed_dim, depths, heads, default_sd: float, **kw) -> SwinTransformer:
    if kw.get("stochastic_depth_prob") is None:
        kw["stochastic_depth_prob"] = default_sd
    return SwinTransformer(embed_dim, depths, heads, **kw)


def swin_t(**kw) -> SwinTransformer:
    return _swin(96, (2, 2, 6, 2), (3, 6, 12, 24), 0.2, **kw)


def swin_s(**kw) -> SwinTransformer:
    return _swin(96, (2, 2, 18, 2), (3, 6, 12, 24), 0.3, **kw)


def swin_b(**kw) -> SwinTransformer:
    return _swin(128, (2, 2, 18, 2), (4, 8, 16, 32), 0.5, **kw)


def swin_nano(**kw) -> SwinTransformer:
    """Embed 32, depths 2-2-2, heads 1-2-4: the variant the tests run, on 112 x 112 images (stage
    maps 28, 14 and 7; no stochastic depth unless asked for)."""
    return _swin(32, (2, 2, 2), (1, 2, 4), 0.0, **kw)


for _name, _fn in (("swin_t", swin_t), ("swin_s", swin_s), ("swin_b", swin_b),
                   ("swin_nano", swin_nano)):
    register_model(_name, _fn)
