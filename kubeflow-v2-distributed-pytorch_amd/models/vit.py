"""Vision Transformer (torchvision's ``vit_b_16`` / ``vit_b_32`` / ``vit_l_16`` / ``vit_l_32``) on
mipipe's transformer kernels.

The module tree and ``state_dict`` keys are torchvision's (``class_token``, ``conv_proj.*``,
``encoder.pos_embedding``, ``encoder.layers.encoder_layer_N.{ln_1, self_attention, ln_2, mlp}``,
``encoder.ln``, ``heads.head``), so checkpoints interchange; ``self_attention.in_proj_weight`` is
``nn.MultiheadAttention``'s packed q | k | v parameter, which is the layout the attention kernel
reads, so no hooks are involved.

Execution (``forward``), every step a HIP kernel:

* patch embedding: ``conv_proj`` is a P x P stride-P convolution, i.e. a GEMM with K = C*P*P
  behind a permutation of the image — :func:`MF.patchify` writes the image as GEMM rows in the
  column order of ``conv_proj.weight.view(D, -1)``, so the parameter is the weight operand as it
  stands and its gradient lands in the flat bucket through the Linear path;
* :func:`MF.tokens_assemble` prepends the class token and adds the position embedding;
* the encoder is pre-LN: the sum ``x + residual`` is normalised AND carried on.
  :func:`MF.add_layer_norm` returns both from one kernel and adds the stream's gradient to the
  LayerNorm's in one backward pass, so a block's two residual adds never run as launches of their
  own;
* flash attention on the packed QKV projection (head_dim 64), the GELU-epilogue GEMM, fused
  cross-entropy: as BERT.

Only the class token's row feeds the head, so the final ``encoder.ln`` runs on those B rows.
Dropout and attention dropout are 0 (torchvision's defaults); position embeddings are not
interpolated: the image size is fixed at construction.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as tnn
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.ops import functional as MF

from . import register_model

_HEAD_DIM = 64  # the attention kernel's head width


class _PatchProj(mnn.ShadowMixin, tnn.Module):
    """``conv_proj``: the state of ``nn.Conv2d(C, D, P, stride=P)`` (weight kept NCHW-contiguous),
    executed as a Linear over patch rows."""

    def __init__(self, in_chans: int, hidden: int, patch: int):
        super().__init__()
        self.in_channels, self.out_channels, self.patch = in_chans, hidden, patch
        self.weight = tnn.Parameter(torch.empty(hidden, in_chans, patch, patch))
        self.bias = tnn.Parameter(torch.zeros(hidden))

    def operand_view(self, w: torch.Tensor) -> torch.Tensor:
        return w.reshape(w.shape[0], -1)  # [D, C*P*P], columns (c, u, v): a view

    def forward(self, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """x [B, C, H, W] -> patch embeddings [B*gh*gw, D] in ``dtype`` (bias included)."""
        tok = MF.patchify(x, self.patch, dtype)
        return MF.linear(tok, self.weight, self.compute_weight(dtype), self.bias)

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.patch}, "
                f"stride={self.patch}")


class _SelfAttention(mnn.ShadowMixin, tnn.Module):
    """The state of ``nn.MultiheadAttention(D, heads, batch_first=True)``: packed
    ``in_proj_weight`` [3D, D] / ``in_proj_bias`` in q | k | v row blocks, and ``out_proj``."""

    def __init__(self, hidden: int, heads: int):
        super().__init__()
        self.embed_dim, self.num_heads = hidden, heads
        self.in_proj_weight = tnn.Parameter(torch.empty(3 * hidden, hidden))
        self.in_proj_bias = tnn.Parameter(torch.zeros(3 * hidden))
        self.out_proj = mnn.Linear(hidden, hidden)

    @property
    def weight(self) -> torch.Tensor:  # the parameter whose shadow ShadowMixin serves
        return self.in_proj_weight

    def forward(self, y: torch.Tensor, B: int, S: int, bias_slot=None) -> torch.Tensor:
        qkv = MF.linear(y, self.in_proj_weight, self.compute_weight(y.dtype), self.in_proj_bias)
        ctx = MF.attention(qkv, B, S, self.num_heads)
        return self.out_proj(ctx, bias_slot=bias_slot)


class _MLP(tnn.Sequential):
    """torchvision's ``MLPBlock``: Linear, GELU, Dropout, Linear, Dropout (keys ``0`` and ``3``)."""

    def __init__(self, hidden: int, mlp_dim: int):
        super().__init__(mnn.Linear(hidden, mlp_dim), tnn.GELU(), tnn.Dropout(0.0),
                         mnn.Linear(mlp_dim, hidden), tnn.Dropout(0.0))


class EncoderBlock(tnn.Module):
    def __init__(self, hidden: int, heads: int, mlp_dim: int, eps: float):
        super().__init__()
        self.ln_1 = mnn.LayerNorm(hidden, eps=eps)
        self.self_attention = _SelfAttention(hidden, heads)
        self.ln_2 = mnn.LayerNorm(hidden, eps=eps)
        self.mlp = _MLP(hidden, mlp_dim)


class _Encoder(tnn.Module):
    def __init__(self, seq: int, layers: int, hidden: int, heads: int, mlp_dim: int, eps: float):
        super().__init__()
        self.pos_embedding = tnn.Parameter(torch.empty(1, seq, hidden).normal_(std=0.02))
        self.layers = tnn.Sequential(OrderedDict(
            (f"encoder_layer_{i}", EncoderBlock(hidden, heads, mlp_dim, eps))
            for i in range(layers)))
        self.ln = mnn.LayerNorm(hidden, eps=eps)


class VisionTransformer(tnn.Module):
    """``forward(x)``: x [B, C, H, W] (NCHW, fp32 or bf16) -> logits [B, num_classes] on mipipe's
    kernels; ``reference_forward(x)``: the same parameters through plain torch."""

    def __init__(self, patch_size: int, num_layers: int, num_heads: int, hidden_dim: int,
                 mlp_dim: int, num_classes: int = 1000, image_size: int = 224, in_chans: int = 3,
                 compute_dtype: Optional[torch.dtype] = None):
        super().__init__()
        if hidden_dim % num_heads or hidden_dim // num_heads != _HEAD_DIM:
            raise ValueError(
                f"VisionTransformer: hidden_dim / num_heads must be {_HEAD_DIM} (the attention "
                f"kernel's head width), got {hidden_dim} / {num_heads}; vit_h_14 (head width 80) "
                "is not supported")
        if patch_size % 8:
            raise ValueError(f"VisionTransformer: the patch size must be a multiple of 8 (the "
                             f"patch kernel's vector width), got {patch_size}")
        if image_size % patch_size:
            raise ValueError(f"VisionTransformer: image size {image_size} is not a multiple of "
                             f"the patch size {patch_size}")
        self.patch_size, self.image_size, self.in_chans = patch_size, image_size, in_chans
        self.hidden_dim, self.num_heads, self.eps = hidden_dim, num_heads, 1e-6
        self.compute_dtype = compute_dtype
        self.class_token = tnn.Parameter(torch.zeros(1, 1, hidden_dim))
        self.conv_proj = _PatchProj(in_chans, hidden_dim, patch_size)
        self.seq_length = (image_size // patch_size) ** 2 + 1
        self.encoder = _Encoder(self.seq_length, num_layers, hidden_dim, num_heads, mlp_dim,
                                self.eps)
        self.heads = tnn.Sequential(OrderedDict(head=mnn.Linear(hidden_dim, num_classes)))
        self._init_weights()
        self._register_load_state_dict_pre_hook(_rename_mlp_keys)

    # torchvision's VisionTransformer / EncoderBlock / MLPBlock / nn.MultiheadAttention inits
    def _init_weights(self):
        cp = self.conv_proj
        fan_in = cp.in_channels * cp.patch * cp.patch
        tnn.init.trunc_normal_(cp.weight, std=math.sqrt(1.0 / fan_in))
        tnn.init.zeros_(cp.bias)
        for blk in self.encoder.layers:
            tnn.init.xavier_uniform_(blk.self_attention.in_proj_weight)
            tnn.init.zeros_(blk.self_attention.in_proj_bias)
            tnn.init.zeros_(blk.self_attention.out_proj.bias)
            for lin in (blk.mlp[0], blk.mlp[3]):
                tnn.init.xavier_uniform_(lin.weight)
                tnn.init.normal_(lin.bias, std=1e-6)
        tnn.init.zeros_(self.heads.head.weight)
        tnn.init.zeros_(self.heads.head.bias)

    def activation_dtype(self, x: torch.Tensor) -> torch.dtype:
        if self.compute_dtype is not None:
            return self.compute_dtype
        return torch.bfloat16 if x.is_cuda else torch.float32

    def _check_input(self, x: torch.Tensor):
        if x.dim() != 4 or x.shape[1] != self.in_chans:
            raise ValueError(f"VisionTransformer: expected [B, {self.in_chans}, H, W] input, got "
                             f"{tuple(x.shape)}")
        H, W, P = x.shape[2], x.shape[3], self.patch_size
        if H % P or W % P:
            raise ValueError(f"VisionTransformer: image {H}x{W} is not a multiple of the patch "
                             f"size {P}")
        if (H // P) * (W // P) + 1 != self.seq_length:
            raise ValueError(
                f"VisionTransformer: image {H}x{W} gives {(H // P) * (W // P)} patches but "
                f"pos_embedding holds {self.seq_length - 1} (built for image_size="
                f"{self.image_size}); position embeddings are not interpolated — construct the "
                "model with the image size you train on")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_input(x)
        dt = self.activation_dtype(x)
        if x.is_cuda and dt != torch.bfloat16:
            raise ValueError(
                f"VisionTransformer: compute dtype {dt} on the GPU is not supported — the "
                "LayerNorm and attention kernels are bf16 (use compute_dtype=torch.bfloat16)")
        B, S, enc = x.shape[0], self.seq_length, self.encoder
        e = self.conv_proj(x, dt)
        h = MF.tokens_assemble(e, self.class_token, enc.pos_embedding)  # [B*S, D]
        blocks = list(enc.layers)
        y = blocks[0].ln_1(h)
        for i, blk in enumerate(blocks):
            # each Linear that feeds an add_layer_norm leaves its bias gradient to that kernel
            s_a, s_f = MF.BiasGradSlot(), MF.BiasGradSlot()
            a = blk.self_attention(y, B, S, bias_slot=s_a)
            y2, h1 = MF.add_layer_norm(a, h, blk.ln_2.weight, blk.ln_2.bias, self.eps, s_a)
            last = i + 1 == len(blocks)
            f = blk.mlp[3](blk.mlp[0](y2, act="gelu"), bias_slot=None if last else s_f)
            if not last:  # the block's closing add runs inside the next block's ln_1
                nxt = blocks[i + 1].ln_1
                y, h = MF.add_layer_norm(f, h1, nxt.weight, nxt.bias, self.eps, s_f)
        # only the class token's row reaches the head: the last closing add and encoder.ln run on
        # those B rows (views of row 0 of every sample; the backward is a slice, no index-add)
        D = self.hidden_dim
        f0 = f.view(B, S, D)[:, 0].contiguous()
        h0 = h1.view(B, S, D)[:, 0].contiguous()
        yc, _ = MF.add_layer_norm(f0, h0, enc.ln.weight, enc.ln.bias, self.eps)
        return self.heads.head(yc)

    def reference_forward(self, x: torch.Tensor) -> torch.Tensor:
        """The same parameters through plain torch: ``F.conv2d`` patch embedding,
        ``F.multi_head_attention_forward`` on the packed projection, ``F.layer_norm``, exact GELU."""
        self._check_input(x)
        B, D, enc = x.shape[0], self.hidden_dim, self.encoder
        cp = self.conv_proj
        e = F.conv2d(x.to(cp.weight.dtype), cp.weight, cp.bias, stride=self.patch_size)
        e = e.reshape(B, D, -1).permute(0, 2, 1)
        h = torch.cat([self.class_token.expand(B, -1, -1), e], 1) + enc.pos_embedding
        for blk in enc.layers:
            sa = blk.self_attention
            y = F.layer_norm(h, (D,), blk.ln_1.weight, blk.ln_1.bias, self.eps).transpose(0, 1)
            a, _ = F.multi_head_attention_forward(
                y, y, y, D, self.num_heads, sa.in_proj_weight, sa.in_proj_bias, None, None, False,
                0.0, sa.out_proj.weight, sa.out_proj.bias, training=False, need_weights=False)
            h = h + a.transpose(0, 1)
            y = F.layer_norm(h, (D,), blk.ln_2.weight, blk.ln_2.bias, self.eps)
            y = F.gelu(F.linear(y, blk.mlp[0].weight, blk.mlp[0].bias))
            h = h + F.linear(y, blk.mlp[3].weight, blk.mlp[3].bias)
        h = F.layer_norm(h, (D,), enc.ln.weight, enc.ln.bias, self.eps)
        return F.linear(h[:, 0], self.heads.head.weight, self.heads.head.bias)


def _rename_mlp_keys(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                     error_msgs):
    """Checkpoints written before torchvision 0.13 name the MLP's Linears ``linear_1`` /
    ``linear_2`` instead of ``0`` / ``3``."""
    for k in list(state_dict.keys()):
        for old, new in ((".mlp.linear_1.", ".mlp.0."), (".mlp.linear_2.", ".mlp.3.")):
            if k.startswith(prefix) and old in k:
                state_dict[k.replace(old, new)] = state_dict.pop(k)


def _vit(patch_size, num_layers, num_heads, hidden_dim, mlp_dim, **kw) -> VisionTransformer:
    return VisionTransformer(patch_size, num_layers, num_heads, hidden_dim, mlp_dim, **kw)


def vit_b_16(**kw) -> VisionTransformer:
    return _vit(16, 12, 12, 768, 3072, **kw)


def vit_b_32(**kw) -> VisionTransformer:
    return _vit(32, 12, 12, 768, 3072, **kw)


def vit_l_16(**kw) -> VisionTransformer:
    return _vit(16, 24, 16, 1024, 4096, **kw)


def vit_l_32(**kw) -> VisionTransformer:
    return _vit(32, 24, 16, 1024, 4096, **kw)


def vit_tiny(**kw) -> VisionTransformer:
    """2 layers, hidden 256 (an exact LayerNorm width), 4 heads, MLP 512, patch 16 on 64 x 64
    images: the variant the tests run."""
    kw.setdefault("image_size", 64)
    kw.setdefault("patch_size", 16)
    return _vit(kw.pop("patch_size"), 2, 4, 256, 512, **kw)


# vit_h_14 (head width 80, patch 14) is deliberately not registered: the attention kernel serves
# head width 64 and the patch kernel multiples of 8
for _name, _fn in (("vit_b_16", vit_b_16), ("vit_b_32", vit_b_32), ("vit_l_16", vit_l_16),
                   ("vit_l_32", vit_l_32), ("vit_tiny", vit_tiny)):
    register_model(_name, _fn)
