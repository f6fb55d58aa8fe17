"""Reference (plain PyTorch) implementations of mipipe's kernel contracts.

Every hot op of the training step is a hand-written HIP kernel on the MI355X
(``csrc/kernels/*.hip`` -> ``mipipe._C``).  This module implements the *same contracts*
(same arguments, layouts, outputs) with ATen math.  It is used

* as the CPU execution path (CPU/gloo configs, tests without a GPU), and
* as the fp32 numerics oracle the GPU tests compare each kernel against.

Layout conventions shared with the kernels: activations are NHWC (``[N, H, W, C]``,
C contiguous); conv weights are ``[Cout, KH, KW, Cin]`` (the channels_last physical order of
a torch ``[Cout, Cin, KH, KW]`` parameter); BN statistics are per channel.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor


def _f(t: Tensor) -> Tensor:
    """Upcast low-precision tensors to fp32; keep fp64 (used by exactness tests)."""
    return t if t.dtype == torch.float64 else t.float()


def _nchw(x: Tensor) -> Tensor:
    return x.permute(0, 3, 1, 2)


def _nhwc(x: Tensor) -> Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def _w_oihw(w: Tensor) -> Tensor:
    return w.permute(0, 3, 1, 2)


def conv_fwd(x: Tensor, w: Tensor, stride: int, pad: int,
             stats_shift: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """y = conv(x, w).  Returns (y, Σ(y-shift), Σ(y-shift)²) per channel ([1, Co] fp32 partials)
    when ``stats_shift`` is given (BN-stat epilogue), else (y, None, None)."""
    yf = F.conv2d(_f(_nchw(x)), _f(_w_oihw(w)), stride=stride, padding=pad)
    y = _nhwc(yf)
    if stats_shift is None:
        return y.to(x.dtype), None, None
    d = y.reshape(-1, y.shape[-1]) - _f(stats_shift)[None, :]
    return y.to(x.dtype), d.sum(0, keepdim=True), (d * d).sum(0, keepdim=True)


def conv_fwd_infer(x: Tensor, w: Tensor, stride, pad, scale: Optional[Tensor] = None,
                   shift: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                   relu: bool = False) -> Tensor:
    """Inference forward (csrc/kernels/conv_infer.hip's contract), NHWC:
    ``act(conv(x, w) * scale[c] + shift[c] + residual)`` in fp32 (float64 for float64 inputs),
    rounded once to ``x``'s dtype.  ``scale`` / ``shift`` absent = 1 / 0."""
    y = _nhwc(F.conv2d(_f(_nchw(x)), _f(_w_oihw(w)), stride=stride, padding=pad))
    if scale is not None:
        y = y * scale.to(y.dtype)
    if shift is not None:
        y = y + shift.to(y.dtype)
    if residual is not None:
        y = y + residual.to(y.dtype)
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


def bn_fold_affine(weight: Tensor, bias: Tensor, running_mean: Tensor, running_var: Tensor,
                   eps: float, conv_bias: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Eval-mode BatchNorm of ``conv + conv_bias`` as a per-channel affine:
    ``scale = γ·rsqrt(var + eps)``, ``shift = β + (conv_bias − mean)·scale``."""
    scale = _f(weight) * torch.rsqrt(_f(running_var) + eps)
    d = -_f(running_mean) if conv_bias is None else _f(conv_bias) - _f(running_mean)
    return scale, _f(bias) + d * scale


def conv_dgrad(dy: Tensor, w: Tensor, x_shape, stride: int, pad: int) -> Tensor:
    N, H, W, Ci = x_shape
    dx = torch.nn.grad.conv2d_input((N, Ci, H, W), _f(_w_oihw(w)), _f(_nchw(dy)),
                                    stride=stride, padding=pad)
    return _nhwc(dx).to(dy.dtype)


def conv_wgrad(dy: Tensor, x: Tensor, kh: int, kw: int, stride: int, pad: int) -> Tensor:
    Co = dy.shape[-1]
    Ci = x.shape[-1]
    dw = torch.nn.grad.conv2d_weight(_f(_nchw(x)), (Co, Ci, kh, kw), _f(_nchw(dy)),
                                     stride=stride, padding=pad)
    return dw.permute(0, 2, 3, 1).contiguous()  # [Co, KH, KW, Ci] fp32


def bn_finalize(psum: Tensor, psumsq: Tensor, count: int, shift: Tensor, gamma: Tensor,
                beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
                momentum: float, eps: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Batch statistics from shifted partial sums; updates running stats in place
    (unbiased variance, torch semantics).  Returns (mean, invstd, scale, bias) with
    ``bn(y) = y*scale + bias``."""
    s = _f(psum).sum(0)
    ss = _f(psumsq).sum(0)
    m_shift = s / count
    var = (ss / count - m_shift * m_shift).clamp_min(0.0)
    mean = m_shift + _f(shift)
    invstd = torch.rsqrt(var + eps)
    scale = _f(gamma) * invstd
    bias = _f(beta) - mean * scale
    if running_mean is not None:
        with torch.no_grad():
            unbiased = var * (count / max(count - 1, 1))
            running_mean.mul_(1 - momentum).add_(mean.to(running_mean.dtype), alpha=momentum)
            running_var.mul_(1 - momentum).add_(unbiased.to(running_var.dtype), alpha=momentum)
    return mean, invstd, scale, bias


def bn_act_fwd(y: Tensor, scale: Tensor, bias: Tensor, relu: bool,
               residual: Optional[Tensor] = None, res_scale: Optional[Tensor] = None,
               res_bias: Optional[Tensor] = None) -> Tensor:
    """z = act(y*scale + bias [+ residual | + residual*res_scale + res_bias])."""
    z = _f(y) * scale + bias
    if residual is not None:
        r = _f(residual)
        if res_scale is not None:
            r = r * res_scale + res_bias
        z = z + r
    if relu:
        z = torch.relu(z)
    return z.to(y.dtype)


def bn_act_bwd_reduce(dz: Tensor, z: Tensor, y: Tensor, mean: Tensor, invstd: Tensor,
                      relu: bool) -> Tuple[Tensor, Tensor]:
    """Σ g and Σ g·x̂ per channel, g = dz·[z>0] (relu) or dz, x̂ = (y-mean)·invstd."""
    C = y.shape[-1]
    g = _f(dz).reshape(-1, C)
    if relu:
        g = g * (z.reshape(-1, C) > 0)
    xhat = (_f(y).reshape(-1, C) - mean) * invstd
    return g.sum(0), (g * xhat).sum(0)


def bn_act_bwd_apply(dz: Tensor, z: Tensor, y: Tensor, mean: Tensor, invstd: Tensor,
                     gamma: Tensor, sum_g: Tensor, sum_gx: Tensor, count: int, relu: bool,
                     want_dres: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """dy = γ·invstd·(g − Σg/n − x̂·Σgx̂/n); optionally d(residual) = g."""
    shp = y.shape
    C = shp[-1]
    g = _f(dz).reshape(-1, C)
    if relu:
        g = g * (z.reshape(-1, C) > 0)
    xhat = (_f(y).reshape(-1, C) - mean) * invstd
    dy = (_f(gamma) * invstd) * (g - sum_g / count - xhat * (sum_gx / count))
    dres = g.reshape(shp).to(dz.dtype) if want_dres else None
    return dy.reshape(shp).to(dz.dtype), dres


def relu_mask_grad(dz: Tensor, z: Tensor) -> Tensor:
    return (_f(dz) * (z > 0)).to(dz.dtype)


def maxpool_fwd(x: Tensor, k: int, stride: int, pad: int,
                ceil_mode: bool = False) -> Tuple[Tensor, Tensor]:
    yf, idx = F.max_pool2d(_f(_nchw(x)), k, stride, pad, ceil_mode=ceil_mode,
                           return_indices=True)
    return _nhwc(yf).to(x.dtype), _nhwc(idx.to(torch.int32))


def maxpool_bwd(dy: Tensor, idx: Tensor, x_shape) -> Tensor:
    N, H, W, C = x_shape
    dyf = _f(_nchw(dy)).reshape(N, C, -1)
    dx = torch.zeros(N, C, H * W, dtype=dyf.dtype, device=dy.device)
    dx.scatter_add_(2, _nchw(idx).reshape(N, C, -1).long(), dyf)
    return _nhwc(dx.reshape(N, C, H, W)).to(dy.dtype)


def avgpool_fwd(x: Tensor) -> Tensor:
    """Global average pool NHWC -> [N, C]."""
    return _f(x).mean(dim=(1, 2)).to(x.dtype)


def avgpool_bwd(dy: Tensor, x_shape) -> Tensor:
    N, H, W, C = x_shape
    return (_f(dy)[:, None, None, :] / (H * W)).expand(N, H, W, C).contiguous().to(dy.dtype)


def gemm(a: Tensor, b: Tensor, trans_a: bool, trans_b: bool, bias: Optional[Tensor] = None,
         act: str = "none", out_dtype=None, c: Optional[Tensor] = None,
         beta: float = 0.0) -> Tensor:
    """C = op(A)·op(B) (+bias per column) (+act) (+beta·C).  A: [M,K] or [K,M]."""
    A = _f(a).t() if trans_a else _f(a)
    B = _f(b).t() if trans_b else _f(b)
    out = A @ B
    if bias is not None:
        out = out + _f(bias)
    if act == "relu":
        out = torch.relu(out)
    elif act == "gelu":
        out = F.gelu(out)
    if c is not None and beta != 0.0:
        out = out + beta * _f(c)
    return out.to(out_dtype or a.dtype)


def cross_entropy_fwd_bwd(logits: Tensor, labels: Tensor, label_smoothing: float = 0.0,
                          ignore_index: int = -100,
                          valid_cols: int = -1) -> Tuple[Tensor, Tensor]:
    """Mean CE over non-ignored rows and its gradient wrt logits (for grad_output = 1).
    ``valid_cols`` > 0: only the first columns are classes; the gradient of the rest is 0.
    A label other than ``ignore_index`` that is outside the classes reads nothing, as in the
    pair-target form: its logit counts as 0 (the row's loss is its log-sum-exp), no column gets
    the ``1 - label_smoothing`` target, and the row still counts in the mean."""
    V = logits.shape[-1]
    if 0 < valid_cols < V:
        loss, g = cross_entropy_fwd_bwd(logits[:, :valid_cols], labels, label_smoothing,
                                        ignore_index)
        return loss, torch.cat([g, g.new_zeros(g.shape[0], V - valid_cols)], 1)
    lf = _f(logits)
    valid = labels != ignore_index
    n = valid.sum().clamp_min(1)
    logp = torch.log_softmax(lf, dim=-1)
    inside = valid & (labels >= 0) & (labels < V)
    safe = torch.where(inside, labels, torch.zeros_like(labels)).long()
    nll = torch.where(inside, -logp.gather(1, safe[:, None])[:, 0], torch.logsumexp(lf, dim=-1))
    if label_smoothing > 0:
        smooth = -logp.mean(dim=-1)
        nll = (1 - label_smoothing) * nll + label_smoothing * smooth
    loss = torch.where(valid, nll, torch.zeros_like(nll)).sum() / n
    p = logp.exp()
    oh = F.one_hot(safe, lf.shape[-1]).float() * inside[:, None]
    if label_smoothing > 0:
        oh = oh * (1 - label_smoothing) + label_smoothing / lf.shape[-1]
    grad = (p - oh) * valid[:, None] / n
    return loss, grad.to(logits.dtype)


def cross_entropy_mixed_fwd_bwd(logits: Tensor, labels: Tensor, mix: Tensor,
                                label_smoothing: float = 0.0,
                                valid_cols: int = -1) -> Tuple[Tensor, Tensor]:
    """Pair-target CE (Mixup / CutMix) and its gradient wrt logits (for grad_output = 1).  Row
    ``r`` of ``R`` has the labels ``a = labels[r]`` and ``b = labels[R-1-r]``; with ``lam =
    mix[0]`` (the batch-mix descriptor, :mod:`mipipe.data.mix`) and ``eps = label_smoothing``
    the target is ``t[c] = eps/Vv + (1-eps) * (lam*[c==a] + (1-lam)*[c==b])`` and the loss the
    mean over all rows of ``lse - sum(t * x)``.  There is no ``ignore_index`` in this form: every
    row counts.  A label outside the classes reads nothing: it matches no column.
    ``valid_cols`` as in :func:`cross_entropy_fwd_bwd`."""
    V = logits.shape[-1]
    if 0 < valid_cols < V:
        loss, g = cross_entropy_mixed_fwd_bwd(logits[:, :valid_cols], labels, mix,
                                              label_smoothing)
        return loss, torch.cat([g, g.new_zeros(g.shape[0], V - valid_cols)], 1)
    lf = _f(logits)
    R = lf.shape[0]
    lam = mix.reshape(-1)[0].to(lf.dtype)
    a = labels.long()
    b = a.flip(0)
    cols = torch.arange(V, device=lf.device)
    t = lam * (cols == a[:, None]).to(lf.dtype) + (1 - lam) * (cols == b[:, None]).to(lf.dtype)
    t = t * (1 - label_smoothing) + label_smoothing / V
    logp = torch.log_softmax(lf, dim=-1)
    # lse - sum(t * x): -sum(t * logp) while the labels are classes (sum(t) = 1); a label that
    # is none takes its weight's logit as 0.  A column without target weight enters nothing (a
    # masked class: 0 * -inf would be nan).
    tx = torch.where(t != 0, t * lf, torch.zeros_like(lf)).sum(-1)
    loss = (torch.logsumexp(lf, dim=-1) - tx).sum() / max(1, R)
    grad = (logp.exp() - t) / max(1, R)
    return loss, grad.to(logits.dtype)


def batch_mix(x: Tensor, mix: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Mixup / CutMix of ``x`` [B, C, H, W] (fp32 or bf16) with its own reverse — sample ``i`` is
    paired with ``B-1-i`` — as the descriptor ``mix`` says (csrc/kernels/mix.hip's contract;
    layout in :mod:`mipipe.data.mix`: ``[lam, mode, y0, y1, x0, x1, 0, 0]``).

    * mode 0: ``out = x``; with ``out is x`` nothing is written.
    * mode 1: ``out[i] = lam*x[i] + (1-lam)*x[B-1-i]`` in fp32: two rounded multiplies and one
      rounded add, ``1-lam`` an fp32 subtraction, rounded once to ``x``'s type.
    * mode 2: ``out[i] = x[B-1-i]`` inside the half-open box, ``x[i]`` outside.
    * The middle sample of an odd batch is its own partner and keeps its bits in every mode
      (``lam*a + (1-lam)*a`` is ``a``; the rounded sum would only be near it).

    ``out``: ``x`` itself (in place), another tensor of the same shape and type, or None (new).
    This reference reads the descriptor on the host; the kernel reads it on the device."""
    B, C, H, W = x.shape
    v = mix.reshape(-1)[:8].tolist()
    mode = int(v[1]) if int(v[1]) in (1, 2) else 0
    if mode == 0:
        if out is None:
            return x.clone()
        if out is not x:
            out.copy_(x)
        return out
    rev = x.flip(0)
    if mode == 1:
        lam = mix.reshape(-1)[0].float()
        om = 1 - lam  # fp32
        p = x.float() * lam
        q = rev.float() * om
        res = (p + q).to(x.dtype)
        if B % 2:
            res[B // 2] = x[B // 2]
    else:
        y0 = min(max(int(v[2]), 0), H)
        y1 = min(max(int(v[3]), y0), H)
        x0 = min(max(int(v[4]), 0), W)
        x1 = min(max(int(v[5]), x0), W)
        res = x.clone()
        res[:, :, y0:y1, x0:x1] = rev[:, :, y0:y1, x0:x1]
    if out is None:
        return res
    out.copy_(res)
    return out


def sgd_step(param: Tensor, grad: Tensor, mom: Tensor, shadow: Optional[Tensor], lr: float,
             momentum: float, dampening: float, weight_decay: float, nesterov: bool,
             first_step: bool, grad_scale: float = 1.0) -> None:
    """torch.optim.SGD semantics ([torch] optim/sgd.py:354-380) on flat buffers; also refreshes
    the bf16 compute shadow of the parameters."""
    g = _f(grad) * grad_scale
    if weight_decay != 0:
        g = g + weight_decay * param
    if momentum != 0:
        if first_step:
            mom.copy_(g)
        else:
            mom.mul_(momentum).add_(g, alpha=1 - dampening)
        g = g + momentum * mom if nesterov else mom
    param.add_(g, alpha=-lr)
    if shadow is not None:
        shadow.copy_(param.to(shadow.dtype))


def adamw_step(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor,
               shadow: Optional[Tensor], lr: float, beta1: float, beta2: float, eps: float,
               weight_decay: float, step: int, grad_scale: float = 1.0) -> None:
    g = _f(grad) * grad_scale
    param.mul_(1 - lr * weight_decay)
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(eps)
    param.addcdiv_(exp_avg, denom, value=-lr / bc1)
    if shadow is not None:
        shadow.copy_(param.to(shadow.dtype))


# ---- large-batch optimizers: the contract of csrc/kernels/optim.hip, written per tensor (no flat
# layout, no chunks) and in the tensors' own dtype, so the same code is the fp32 CPU path and,
# given float64 tensors, the oracle of the GPU tests.

def lr_schedule(kind: str, base_lr: float, warmup_steps: int, total_steps: int, end_lr: float,
                k: int) -> float:
    """Learning rate of step ``k`` (from 0), in double precision: ``base·(k+1)/W`` for ``k < W``,
    then from ``base`` to ``end`` over ``x = (k−W)/(T−W)`` clamped to [0, 1]."""
    W, T = int(warmup_steps), int(total_steps)
    if k < W:
        return base_lr * (k + 1) / W
    if kind == "constant":
        return base_lr
    x = min(1.0, (k - W) / (T - W)) if T > W else 1.0
    if kind == "linear":
        f = 1.0 - x
    elif kind == "poly":
        f = (1.0 - x) ** 2
    elif kind == "cosine":
        f = 0.5 * (1.0 + math.cos(math.pi * x))
    else:
        raise ValueError(f"unknown LR schedule '{kind}'")
    return end_lr + (base_lr - end_lr) * f


def clip_coef(grads, grad_scale: float = 1.0, max_norm: Optional[float] = None):
    """(‖g·grad_scale‖ over all tensors, clip) with torch.nn.utils.clip_grad_norm_'s rule
    ``clip = min(1, max_norm / (norm + 1e-6))``; ``max_norm=None``: clip = 1."""
    tot = sum(((g * grad_scale) ** 2).sum() for g in grads)
    norm = torch.sqrt(tot)
    if max_norm is None:
        return norm, torch.ones_like(norm)
    return norm, torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def lars_step(w: Tensor, g: Tensor, m: Tensor, lr: float, momentum: float, weight_decay: float,
              trust_coefficient: Optional[float], eps: float, adapt: bool,
              grad_scale=1.0) -> Tensor:
    """One tensor's LARS update in place (LARC-style composition); returns the trust ratio.
    ``g' = g·grad_scale`` (``grad_scale`` already holds the clip coefficient);
    ``r = tc·‖w‖ / (‖g'‖ + wd·‖w‖ + eps)`` if adapted and both norms > 0, else 1;
    ``d = r·(g' + wd·w)``; ``m = μ·m + d``; ``w −= lr·m``.  With r = 1 this is plain SGD."""
    gp = g * grad_scale
    r = torch.ones((), dtype=w.dtype, device=w.device)
    if adapt and trust_coefficient is not None:
        wn, gn = w.norm(), gp.norm()
        if wn > 0 and gn > 0:
            r = trust_coefficient * wn / (gn + weight_decay * wn + eps)
    d = r * (gp + weight_decay * w)
    m.mul_(momentum).add_(d)
    w.sub_(lr * m)
    return r


def lamb_step(w: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, beta1: float, beta2: float,
              eps: float, weight_decay: float, step: int, adapt: bool, grad_scale=1.0) -> Tensor:
    """One tensor's LAMB update in place; returns the trust ratio.  ``step`` counts from 1.
    ``u = (m/(1−β1ᵗ)) / (√(v/(1−β2ᵗ)) + eps) + wd·w``; ``r = ‖w‖/‖u‖`` if adapted and both
    norms > 0, else 1; ``w −= lr·r·u``."""
    gp = g * grad_scale
    m.mul_(beta1).add_(gp, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gp, gp, value=1 - beta2)
    u = (m / (1 - beta1 ** step)) / ((v / (1 - beta2 ** step)).sqrt() + eps) + weight_decay * w
    r = torch.ones((), dtype=w.dtype, device=w.device)
    if adapt:
        wn, un = w.norm(), u.norm()
        if wn > 0 and un > 0:
            r = wn / un
    w.sub_(lr * r * u)
    return r


# ---- weight EMA: the contract of csrc/kernels/ema.hip

def ema_weight(calls: int, every: int, w_min, warmup: bool):
    """The averaging weight of ``update()`` call number ``calls`` (from 1) as an fp32 0-d tensor,
    or None when the call is skipped (``calls % every != 0``).  ``u = calls/every − 1`` counts the
    averaging updates from 0; ``w = max(w_min, 9/(10+u))`` with warm-up (timm's
    ``1 − min(decay, (1+u)/(10+u))`` without the cancellation), else ``w_min``; all in fp32, with
    ``w_min = float32(1 − decay)``."""
    if every < 1 or calls < every or calls % every != 0:
        return None
    w = torch.tensor(float(w_min), dtype=torch.float32)
    if warmup:
        u = calls // every - 1
        w = torch.maximum(w, torch.tensor(9.0, dtype=torch.float32)
                          / torch.tensor(float(10 + u), dtype=torch.float32))
    return w


def ema_update(e: Tensor, p: Tensor, w) -> None:
    """``e = e + w·(p − e)`` in place: a rounded subtract, a rounded multiply and a rounded add in
    ``e``'s dtype, ``w`` an fp32 value (a float that fp32 holds exactly, or a 0-d tensor)."""
    w = torch.as_tensor(w, dtype=torch.float32).to(device=e.device, dtype=e.dtype)
    d = p - e
    d.mul_(w)
    e.add_(d)


def ema_swap(p: Tensor, e: Tensor, shadow: Optional[Tensor] = None) -> None:
    """``p' = e``, ``e' = p``, ``shadow' = p'`` rounded to the shadow's type: a pure exchange, so
    two swaps restore all three tensors bit for bit."""
    t = p.clone()
    p.copy_(e)
    e.copy_(t)
    if shadow is not None:
        shadow.copy_(p.to(shadow.dtype))


def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float,
                  residual: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """(y, mean, rstd, x_sum): y = LN(x [+ residual]); x_sum = x+residual (saved for bwd)."""
    xs = _f(x) if residual is None else _f(x) + _f(residual)
    mean = xs.mean(-1)
    var = xs.var(-1, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    y = (xs - mean[..., None]) * rstd[..., None] * _f(gamma) + _f(beta)
    return y.to(x.dtype), mean, rstd, (xs.to(x.dtype) if residual is not None else None)


def layernorm_bwd(dy: Tensor, x: Tensor, mean: Tensor, rstd: Tensor,
                  gamma: Tensor, dsum: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``dsum`` (dx's shape): the gradient of the residual stream a pre-LN block carries past the
    LayerNorm, added to dx before its one rounding; dgamma / dbeta do not depend on it."""
    H = x.shape[-1]
    xf = _f(x).reshape(-1, H)
    g = _f(dy).reshape(-1, H)
    xhat = (xf - mean.reshape(-1, 1)) * rstd.reshape(-1, 1)
    dgamma = (g * xhat).sum(0)
    dbeta = g.sum(0)
    gg = g * _f(gamma)
    dx = rstd.reshape(-1, 1) * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))
    if dsum is not None:
        dx = dx + _f(dsum).reshape(-1, H)
    return dx.reshape(x.shape).to(dy.dtype), dgamma, dbeta


# ---- Vision Transformer input side (csrc/kernels/vit.hip)
def patchify(x: Tensor, patch: int, dtype: torch.dtype) -> Tensor:
    """x [B, C, H, W] -> [B*gh*gw, C*P*P] in ``dtype``: row (b, i, j), column (c, u, v) holds
    ``x[b, c, i*P + u, j*P + v]`` — the column order of ``conv_proj.weight.view(D, C*P*P)``, so the
    P x P stride-P convolution is ``rows @ weight.view(D, -1).T``.  A permutation and a cast."""
    B, C, H, W = x.shape
    P = int(patch)
    if P < 1 or H % P or W % P:
        raise ValueError(f"image {H}x{W} is not a whole number of {P}x{P} patches")
    gh, gw = H // P, W // P
    t = x.reshape(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5)
    return t.reshape(B * gh * gw, C * P * P).to(dtype)


def tokens_assemble_fwd(e: Tensor, cls: Tensor, pos: Tensor) -> Tensor:
    """e [B*N, D] (activation dtype), cls [D], pos [(N+1)*D] (master precision) ->
    h [B*(N+1), D]: ``h[b, 0] = cls + pos[0]``, ``h[b, 1+n] = e[b, n] + pos[1+n]``; one add in the
    master precision, one rounding to e's dtype."""
    D = cls.numel()
    S = pos.numel() // D
    B = e.shape[0] // (S - 1)
    pos = _f(pos).reshape(S, D)
    h = torch.empty(B, S, D, dtype=pos.dtype, device=e.device)
    h[:, 0] = _f(cls).reshape(D) + pos[0]
    h[:, 1:] = _f(e).reshape(B, S - 1, D) + pos[1:]
    return h.reshape(B * S, D).to(e.dtype)


def tokens_assemble_bwd(dh: Tensor, batch: int) -> Tuple[Tensor, Tensor, Tensor]:
    """dh [B*(N+1), D] -> (de [B*N, D] = dh without the class rows, dpos [(N+1)*D] = Σ_b dh[b],
    dcls [D] = Σ_b dh[b, 0]); the sums in fp32 (fp64 for fp64 input)."""
    D = dh.shape[-1]
    g = dh.reshape(batch, -1, D)
    dpos = _f(g).sum(0)
    return g[:, 1:].reshape(-1, D).contiguous(), dpos.reshape(-1), dpos[0].clone()


_M32 = 0xFFFFFFFF


def _mix32(x: Tensor) -> Tensor:
    """murmur3 finaliser on uint32 values held in int64 (bit-exact with the HIP kernels)."""
    x = x & _M32
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def _drop_threshold(p: float) -> int:
    return min(int(p * 4294967296.0), _M32)


def attention_keep(B: int, S: int, H: int, p: float, seed: int, device) -> Tensor:
    """[B,H,S(q),S(k)] keep mask of the attention-probability dropout (attention.hip keep_elem)."""
    q = torch.arange(S, device=device, dtype=torch.int64)
    bh = torch.arange(B * H, device=device, dtype=torch.int64)
    row_id = (bh[:, None] * S + q[None, :]) & _M32                      # [BH, S]
    a = _mix32(torch.full_like(row_id, seed & _M32) ^ ((row_id * 0x9E3779B1) & _M32))
    k = torch.arange(S, device=device, dtype=torch.int64)
    kk = (k * 0x85EBCA77 + 0x27D4EB2F) & _M32
    h = _mix32(a[:, :, None] ^ kk[None, None, :])
    return (h >= _drop_threshold(p)).reshape(B, H, S, S)


def dropout_keep(n: int, p: float, seed: int, device) -> Tensor:
    """flat keep mask of misc.hip dropout_kernel."""
    base = _mix32(torch.tensor(((seed & _M32) * 0x9E3779B1 + 0x7F4A7C15) & _M32, dtype=torch.int64))
    i = torch.arange(n, device=device, dtype=torch.int64)
    h = _mix32(base.to(device) ^ (((i & _M32) * 0x85EBCA77) & _M32))
    return h >= _drop_threshold(p)


def fold_dev_seed(base: int, counter: int) -> int:
    """The host seed that draws the masks of ``DevSeed(base, counter)``: drop_base's mixing of
    the device counter (csrc/kernels/drop_hash.hpp)."""
    v = torch.tensor(((base & _M32) ^ ((counter * 0x9E3779B1 + 0x632BE5AB) & _M32)) & _M32,
                     dtype=torch.int64)
    return int(_mix32(v))


def dropout_fwd(x: Tensor, p: float, seed: int) -> Tensor:
    if p <= 0.0:
        return x.clone()
    keep = dropout_keep(x.numel(), p, seed, x.device).reshape(x.shape)
    return (_f(x) * keep / (1.0 - p)).to(x.dtype)


def _split_qkv(qkv: Tensor, B: int, S: int, H: int):
    x = _f(qkv).reshape(B, S, 3, H, -1)
    return (x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2))


def attention_fwd(qkv: Tensor, B: int, S: int, H: int, mask: Optional[Tensor], scale: float,
                  p_drop: float = 0.0, seed: int = 0) -> Tuple[Tensor, Tensor]:
    """Packed layout of attention.hip: qkv [B*S, 3*H*D] -> (o [B*S, H*D], lse [B,H,S])."""
    q, k, v = _split_qkv(qkv, B, S, H)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if mask is not None:
        s = s + _f(mask).reshape(B, 1, 1, S)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    if p_drop > 0.0:
        p = p * attention_keep(B, S, H, p_drop, seed, qkv.device) / (1.0 - p_drop)
    o = torch.einsum("bhqk,bhkd->bhqd", p, v)
    return o.transpose(1, 2).reshape(B * S, -1).to(qkv.dtype), lse


def attention_bwd(do: Tensor, qkv: Tensor, o: Tensor, lse: Tensor, B: int, S: int, H: int,
                  mask: Optional[Tensor], scale: float, p_drop: float = 0.0,
                  seed: int = 0) -> Tensor:
    q, k, v = _split_qkv(qkv, B, S, H)
    D = q.shape[-1]
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if mask is not None:
        s = s + _f(mask).reshape(B, 1, 1, S)
    p = torch.exp(s - lse[..., None])
    dof = _f(do).reshape(B, S, H, D).transpose(1, 2)
    of = _f(o).reshape(B, S, H, D).transpose(1, 2)
    keep = None
    if p_drop > 0.0:
        keep = attention_keep(B, S, H, p_drop, seed, qkv.device) / (1.0 - p_drop)
    pd = p if keep is None else p * keep
    dv = torch.einsum("bhqk,bhqd->bhkd", pd, dof)
    dp = torch.einsum("bhqd,bhkd->bhqk", dof, v)
    if keep is not None:
        dp = dp * keep
    delta = (dof * of).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.einsum("bhqk,bhkd->bhqd", ds, k)
    dk = torch.einsum("bhqk,bhqd->bhkd", ds, q)
    out = torch.stack([t.transpose(1, 2) for t in (dq, dk, dv)], dim=2)  # [B,S,3,H,D]
    return out.reshape(B * S, 3 * H * D).to(qkv.dtype)


def embedding_bwd(dy: Tensor, idx: Tensor, num_rows: int) -> Tensor:
    H = dy.shape[-1]
    src = _f(dy.reshape(-1, H))
    out = torch.zeros(num_rows, H, dtype=src.dtype, device=dy.device)
    out.index_add_(0, idx.reshape(-1).long(), src)
    return out


def gelu_fwd(x: Tensor) -> Tensor:
    return F.gelu(_f(x)).to(x.dtype)


def gelu_bwd(dy: Tensor, x: Tensor) -> Tensor:
    xf = _f(x)
    cdf = 0.5 * (1.0 + torch.erf(xf / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * xf * xf) / math.sqrt(2.0 * math.pi)
    return (_f(dy) * (cdf + xf * pdf)).to(dy.dtype)


# ----------------------------------------------------------------------------- vision.hip
def act_fn(t: Tensor, act: str) -> Tensor:
    if act == "relu":
        return torch.relu(t)
    if act == "relu6":
        return t.clamp(0.0, 6.0)
    return t


def act_keep(z: Tensor, act: str) -> Optional[Tensor]:
    """Where the activation passes gradient, judged from its OUTPUT z like the kernels do
    (relu: z > 0; relu6: 0 < z < 6)."""
    if act == "relu":
        return z > 0
    if act == "relu6":
        return (z > 0) & (z < 6)
    return None


def _masked(dy: Tensor, z: Optional[Tensor], act: str) -> Tensor:
    g = _f(dy)
    keep = None if z is None else act_keep(_f(z), act)
    return g if keep is None else g * keep


def gconv_fwd(x: Tensor, w: Tensor, stride, pad, groups: int, bias: Optional[Tensor] = None,
              act: str = "none") -> Tensor:
    """y = act(conv(x, w, groups) + bias); x NHWC, w [Co, KH, KW, Ci/groups]; stride/pad (h, w)."""
    y = F.conv2d(_f(_nchw(x)), _f(_w_oihw(w)), None if bias is None else _f(bias),
                 stride=tuple(stride), padding=tuple(pad), groups=groups)
    return act_fn(_nhwc(y), act).to(x.dtype)


def gconv_dgrad(dy: Tensor, w: Tensor, x_shape, stride, pad, groups: int,
                z: Optional[Tensor] = None, act: str = "none") -> Tensor:
    N, H, W, Ci = x_shape
    g = _masked(dy, z, act)
    dx = torch.nn.grad.conv2d_input((N, Ci, H, W), _f(_w_oihw(w)), _nchw(g), stride=tuple(stride),
                                    padding=tuple(pad), groups=groups)
    return _nhwc(dx).to(dy.dtype)


def gconv_wgrad(dy: Tensor, x: Tensor, kh: int, kw: int, stride, pad, groups: int,
                z: Optional[Tensor] = None, act: str = "none") -> Tuple[Tensor, Tensor]:
    """(dw [Co, KH, KW, Ci/groups], db [Co]) in fp32 (fp64 inputs stay fp64)."""
    g = _masked(dy, z, act)
    Co, Ci = dy.shape[-1], x.shape[-1]
    dw = torch.nn.grad.conv2d_weight(_f(_nchw(x)), (Co, Ci // groups, kh, kw), _nchw(g),
                                     stride=tuple(stride), padding=tuple(pad), groups=groups)
    return dw.permute(0, 2, 3, 1).contiguous(), g.reshape(-1, Co).sum(0)


def chan_stats(y: Tensor, shift: Tensor) -> Tuple[Tensor, Tensor]:
    """Shifted per-channel sums Σ(y - shift), Σ(y - shift)² ([1, C] each)."""
    C = y.shape[-1]
    d = _f(y).reshape(-1, C) - _f(shift)[None, :]
    return d.sum(0, keepdim=True), (d * d).sum(0, keepdim=True)


def affine_act(y: Tensor, scale: Tensor, bias: Tensor, act: str = "none") -> Tensor:
    return act_fn(_f(y) * scale + bias, act).to(y.dtype)


def bn_generic_bwd_reduce(dz: Tensor, z: Optional[Tensor], y: Tensor, mean: Tensor,
                          invstd: Tensor, act: str = "none") -> Tuple[Tensor, Tensor]:
    """Σg and Σg·x̂ per channel, g = dz·act'(z), x̂ = (y - mean)·invstd."""
    C = y.shape[-1]
    g = _masked(dz, z, act).reshape(-1, C)
    xhat = (_f(y).reshape(-1, C) - mean) * invstd
    return g.sum(0), (g * xhat).sum(0)


def bn_generic_bwd_apply(dz: Tensor, z: Optional[Tensor], y: Tensor, mean: Tensor,
                         invstd: Tensor, gamma: Tensor, sum_g: Optional[Tensor],
                         sum_gx: Optional[Tensor], count: int, act: str = "none") -> Tensor:
    """dy = γ·invstd·(g − Σg/n − x̂·Σgx̂/n); without sums (eval-mode BN) dy = γ·invstd·g."""
    shp = y.shape
    C = shp[-1]
    g = _masked(dz, z, act).reshape(-1, C)
    if sum_g is None:
        dy = (_f(gamma) * invstd) * g
    else:
        xhat = (_f(y).reshape(-1, C) - mean) * invstd
        dy = (_f(gamma) * invstd) * (g - sum_g / count - xhat * (sum_gx / count))
    return dy.reshape(shp).to(dz.dtype)


def avgpool2d_fwd(x: Tensor, k: int, stride: int, pad: int) -> Tensor:
    return _nhwc(F.avg_pool2d(_f(_nchw(x)), k, stride, pad)).to(x.dtype)


def avgpool2d_bwd(dy: Tensor, x_shape, k: int, stride: int, pad: int) -> Tensor:
    N, H, W, C = x_shape
    with torch.enable_grad():
        xz = torch.zeros(N, C, H, W, dtype=_f(dy).dtype, device=dy.device, requires_grad=True)
        yz = F.avg_pool2d(xz, k, stride, pad)
        (g,) = torch.autograd.grad(yz, xz, _f(_nchw(dy)).contiguous())
    return _nhwc(g).to(dy.dtype)


def synthetic_images(indices: Tensor, num_classes: int, shape, seed: int,
                     dtype=torch.float32) -> Tuple[Tensor, Tensor]:
    """Deterministic, *learnable* synthetic NHWC images: label = hash(index) % classes,
    image = class template + unit gaussian noise keyed by (seed, index)."""
    N = indices.numel()
    H, W, C = shape
    idx = indices.long()
    labels = ((idx * 2654435761 + seed * 97) % 2147483647) % num_classes
    g = torch.Generator(device=indices.device)
    g.manual_seed(seed)
    templates = torch.randn(num_classes, H, W, C, generator=g, device=indices.device)
    noise = torch.empty(N, H, W, C, device=indices.device)
    for i in range(N):
        gi = torch.Generator(device=indices.device)
        gi.manual_seed(int(seed) * 7919 + int(idx[i]))
        noise[i] = torch.randn(H, W, C, generator=gi, device=indices.device)
    x = 0.5 * templates[labels] + noise
    return x.to(dtype), labels


def bn_relu_fold(y: Tensor, scale: Tensor, bias: Tensor) -> Tensor:
    """The operand a folded input BatchNorm hands its consumer conv: relu(y*scale + bias) per
    channel (NHWC), in y's dtype — the values bn_act_fwd would have stored."""
    return torch.relu(y.float() * scale.float() + bias.float()).to(y.dtype)


def record_decode(rec: Tensor, idx: Tensor, affine: Tensor, shape, seed: int, epoch: int,
                  pad: int, flip: bool, train: bool, label_bytes: int = 1,
                  dtype=torch.float32) -> Tuple[Tensor, Tensor]:
    """The record loader's transform on whole records (csrc/kernels/records.hip's contract):
    ``rec`` uint8 [n, label_bytes + C*H*W], ``idx`` int64 [n] global sample indices, ``affine``
    fp32 [2, C] (scale row, offset row) -> (x [n, C, H, W] ``dtype``, y [n] int64).  Per-sample
    (dy, dx, flip) are splitmix64 of (seed, epoch, index) as in ``data.records``; the pixel is
    zero outside the image, then ``v * scale`` and ``+ offset`` as two rounded fp32 operations."""
    from mipipe.data.records import _MASK64, _splitmix64
    C, H, W = shape
    n = rec.shape[0]
    dev = rec.device
    y = torch.zeros(n, dtype=torch.int64, device=dev)
    for k in range(label_bytes):
        y |= rec[:, k].long() << (8 * k)
    dy, dx, fl = [0] * n, [0] * n, [False] * n
    if train:
        for s, gi in enumerate(idx.tolist()):
            h = _splitmix64(seed ^ _splitmix64(((epoch * 0x100000001B3) & _MASK64) ^ (gi & _MASK64)))
            if pad > 0:
                dy[s] = int(h % (2 * pad + 1)) - pad
                dx[s] = int((h >> 16) % (2 * pad + 1)) - pad
            fl[s] = bool(flip and ((h >> 40) & 1))
    img = rec[:, label_bytes:].reshape(n, C, H, W).float()
    padded = F.pad(img, (pad, pad, pad, pad))
    ar_h = torch.arange(H, device=dev)
    ar_w = torch.arange(W, device=dev)
    rows = ar_h[None, :] + (torch.tensor(dy, device=dev, dtype=torch.long)[:, None] + pad)
    flt = torch.tensor(fl, device=dev, dtype=torch.bool)[:, None]
    cols = torch.where(flt, (W - 1 - ar_w)[None, :], ar_w[None, :]) \
        + (torch.tensor(dx, device=dev, dtype=torch.long)[:, None] + pad)
    out = padded[torch.arange(n, device=dev)[:, None, None, None],
                 torch.arange(C, device=dev)[None, :, None, None],
                 rows[:, None, :, None], cols[:, None, None, :]]
    sc = affine[0].float().view(1, C, 1, 1)
    off = affine[1].float().view(1, C, 1, 1)
    x = out * sc
    x = x + off
    return x.to(dtype), y


def record_augment(rec: Tensor, idx: Tensor, shape, seed: int, epoch: int, label_bytes: int = 1,
                   force: int = -1) -> Tensor:
    """TrivialAugmentWide on whole records (csrc/kernels/augment.hip's record_augment contract):
    every image through ``data.records.reference_augment``, the label bytes copied."""
    import numpy as np
    from mipipe.data.records import reference_augment
    C, H, W = shape
    src = rec.cpu().numpy()
    out = src.copy()
    for s, gi in enumerate(idx.tolist()):
        img = src[s, label_bytes:].reshape(C, H, W)
        out[s, label_bytes:] = reference_augment(img, gi, epoch, seed, force).reshape(-1)
    return torch.from_numpy(out).to(rec.device)


def batch_erase_(x: Tensor, idx: Tensor, seed: int, epoch: int, pq: int) -> Tensor:
    """Random Erasing in place (csrc/kernels/augment.hip's batch_erase contract): the box of
    ``data.records.reference_erase_box`` of every sample becomes 0.0 in every channel."""
    from mipipe.data.records import reference_erase_box
    Ho, Wo = x.shape[2:]
    for s, gi in enumerate(idx.tolist()):
        box = reference_erase_box(seed, epoch, gi, pq, Ho, Wo)
        if box is not None:
            y0, x0, h, w = box
            x[s, :, y0:y0 + h, x0:x0 + w] = 0
    return x


def record_decode_rrc(rec: Tensor, idx: Tensor, affine: Tensor, shape, out_size, seed: int,
                      epoch: int, flip: bool, train: bool, label_bytes: int = 1,
                      dtype=torch.float32) -> Tuple[Tensor, Tensor]:
    """The record loader's ``"rrc"`` transform on whole records (csrc/kernels/records.hip's
    record_decode_rrc contract): inputs as :func:`record_decode`, x is [n, C, Ho, Wo].  Per sample
    the integer box of ``data.records.reference_rrc_box`` is resampled bilinearly with the Q16
    taps of ``data.records._rrc_taps`` (flip = taps of the mirrored column): the horizontal
    blends are exact, the vertical one is two rounded multiplies and a rounded add, then
    ``v * scale`` and ``+ offset`` — the same bits as ``reference_transform_rrc``."""
    import numpy as np
    from mipipe.data.records import _check_rrc_geometry, _rrc_taps, reference_rrc_box
    C, H, W = shape
    Ho, Wo = out_size
    _check_rrc_geometry(H, W, Ho, Wo)
    n = rec.shape[0]
    dev = rec.device
    y = torch.zeros(n, dtype=torch.int64, device=dev)
    for k in range(label_bytes):
        y |= rec[:, k].long() << (8 * k)
    rows = np.zeros((2, n, Ho), np.int64)
    cols = np.zeros((2, n, Wo), np.int64)
    wy = np.zeros((2, n, Ho), np.float32)
    wx = np.zeros((2, n, Wo), np.float32)
    for s, gi in enumerate(idx.tolist()):
        y0, x0, h, w, fl = reference_rrc_box(seed, epoch, gi, H, W, train, flip)
        r0, r1, l0, l1 = _rrc_taps(h, Ho)
        rows[0, s], rows[1, s], wy[0, s], wy[1, s] = r0 + y0, r1 + y0, l0, l1
        c0, c1, l0, l1 = _rrc_taps(w, Wo)
        if fl:
            c0, c1, l0, l1 = c0[::-1], c1[::-1], l0[::-1], l1[::-1]
        cols[0, s], cols[1, s], wx[0, s], wx[1, s] = c0 + x0, c1 + x0, l0, l1
    rows, cols = torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)
    wy, wx = torch.from_numpy(wy).to(dev), torch.from_numpy(wx).to(dev)
    img = rec[:, label_bytes:].reshape(n, C, H, W).float()
    ar_n = torch.arange(n, device=dev)[:, None, None, None]
    ar_c = torch.arange(C, device=dev)[None, :, None, None]

    def tap(r, c):
        return img[ar_n, ar_c, rows[r][:, None, :, None], cols[c][:, None, None, :]]

    lx0, lx1 = wx[0][:, None, None, :], wx[1][:, None, None, :]
    top = tap(0, 0) * lx0 + tap(0, 1) * lx1
    bot = tap(1, 0) * lx0 + tap(1, 1) * lx1
    a = top * wy[0][:, None, :, None]
    b = bot * wy[1][:, None, :, None]
    v = a + b
    x = v * affine[0].float().view(1, C, 1, 1)
    x = x + affine[1].float().view(1, C, 1, 1)
    return x.to(dtype), y


EVAL_Q24 = float(1 << 24)  # fixed-point scale of the loss and confidence sums
EVAL_LOSS_CAP = float(1 << 16)  # a row loss above this counts as non-finite


def eval_stats(logits: Tensor, labels: Tensor, counters: Tensor,
               confusion: Optional[Tensor] = None, hist: Optional[Tensor] = None, k: int = 5,
               ignore_index: int = -100, valid_cols: int = -1) -> None:
    """Evaluation statistics of logits ``[R, V]`` accumulated into integer buffers
    (csrc/kernels/eval_stats.hip's contract).  ``Vv = valid_cols`` when ``0 < valid_cols < V``,
    else ``V``: only the first ``Vv`` columns are classes, the rest enter no result.

    * ``counters`` int64 [8] += ``[rows, top1, topk, nonfinite, invalid, loss_q24, 0, 0]``;
    * ``confusion`` int32 ``[Vv, Vv]`` (optional): ``confusion[label, pred] += 1``;
    * ``hist`` int64 ``[3, bins]`` (optional): row 0 counts wrong predictions per confidence
      bin, row 1 correct ones, row 2 holds the Q24 sum of the confidences.

    Per row with label ``y``: ``y == ignore_index`` skips the row entirely; ``y < 0`` or
    ``y >= Vv`` counts it in ``invalid`` and nowhere else.  Logits are ordered with NaN above
    every number and NaNs equal to each other.  ``pred`` is the first maximal index
    (``torch.argmax``'s tie rule); ``rank = #{c: x[c] > x[y]} + #{c < y: x[c] == x[y]}``; the
    row is a top-1 hit iff ``pred == y`` (``rank == 0``) and a top-k hit iff ``rank < k``.  The
    loss ``logsumexp(x) - x[y]`` and the confidence ``exp(max - logsumexp)`` are fp32.  A row
    whose loss is not finite or exceeds 2^16 counts in ``nonfinite`` and stays out of the loss sum
    and the histogram (its top-k and confusion entries count); otherwise the loss, clamped at 0,
    and the confidence are rounded to nearest into Q24 and added as integers.  The bin is
    ``min(bins - 1, floor(conf * bins))``."""
    R, V = logits.shape
    Vv = valid_cols if 0 < valid_cols < V else V
    if not 1 <= k <= Vv:
        raise ValueError(f"k must be in [1, {Vv}], got {k}")
    labels = labels.reshape(-1).long()
    keep = labels != ignore_index
    ok = keep & (labels >= 0) & (labels < Vv)
    counters[4] += int((keep & ~ok).sum())
    x = _f(logits[:, :Vv])[ok]
    y = labels[ok]
    n = x.shape[0]
    if n == 0:
        return
    nan = x != x
    has_nan = nan.any(1)
    xy = x.gather(1, y[:, None])
    nan_y = xy != xy
    gt = (x > xy) | (nan & ~nan_y)
    eq = (x == xy) | (nan & nan_y)
    cols = torch.arange(Vv, device=x.device)
    rank = gt.sum(1) + (eq & (cols[None, :] < y[:, None])).sum(1)
    mx = torch.where(nan, torch.full_like(x, float("-inf")), x).max(1).values
    is_max = torch.where(has_nan[:, None], nan, x == mx[:, None])
    pred = is_max.to(torch.uint8).argmax(1)
    hit = pred == y
    lse = torch.logsumexp(x, 1)
    loss = lse - xy[:, 0]
    finite = torch.isfinite(loss) & (loss <= EVAL_LOSS_CAP)
    loss_q = torch.round(loss[finite].clamp_min(0) * EVAL_Q24).to(torch.int64)
    counters[0] += n
    counters[1] += int(hit.sum())
    counters[2] += int((rank < k).sum())
    counters[3] += int((~finite).sum())
    counters[5] += int(loss_q.sum())
    if confusion is not None:
        cm = torch.bincount(y * Vv + pred, minlength=Vv * Vv).reshape(Vv, Vv)
        confusion += cm.to(confusion.dtype)
    if hist is not None:
        bins = hist.shape[1]
        conf = torch.exp(mx - lse)[finite]
        b = torch.floor(conf * bins).clamp(0, bins - 1).to(torch.int64)
        h = hit[finite]
        hist[0] += torch.bincount(b[~h], minlength=bins)
        hist[1] += torch.bincount(b[h], minlength=bins)
        hist[2].index_add_(0, b, torch.round(conf * EVAL_Q24).to(torch.int64))


# ---- ConvNeXt block (csrc/kernels/dwconv7.hip)
def _dw7_w(w: Tensor) -> Tensor:
    """operand [C, 7, 7, 1] -> torch's depthwise filter [C, 1, 7, 7]"""
    return _f(w).permute(0, 3, 1, 2)


def dwconv7_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """Depthwise 7x7, stride 1, pad 3: x [N, H, W, C], w [C, 7, 7, 1] (the operand layout of
    ``gconv``), bias [C] -> y = T(b[c] + sum_{kh,kw} x[n, h+kh-3, w+kw-3, c] * w[c, kh, kw]);
    taps outside the image contribute zero; fp32 accumulation, one rounding."""
    C = x.shape[-1]
    y = F.conv2d(_f(_nchw(x)), _dw7_w(w), None if bias is None else _f(bias), padding=3, groups=C)
    return _nhwc(y).to(x.dtype)


def dwconv7_dgrad(dy: Tensor, w: Tensor, addend: Optional[Tensor] = None) -> Tensor:
    """dx = T(conv(dy, w mirrored) [+ addend]): a stride-1 "same" depthwise data-grad is a forward
    convolution with the taps flipped; ``addend`` (dx's shape: the residual stream's gradient) is
    added in fp32 before the single rounding."""
    C = dy.shape[-1]
    dx = _nhwc(F.conv2d(_f(_nchw(dy)), _dw7_w(w).flip(2, 3), None, padding=3, groups=C))
    if addend is not None:
        dx = dx + _f(addend)
    return dx.to(dy.dtype)


def dwconv7_wgrad(dy: Tensor, x: Tensor) -> Tuple[Tensor, Tensor]:
    """(dw [C, 1, 7, 7], db [C]) in fp32 (fp64 inputs stay fp64):
    dw[c, kh, kw] = sum dy[n, h, w, c] * x[n, h+kh-3, w+kw-3, c], db[c] = sum dy."""
    N, H, W, C = x.shape
    xp = F.pad(_f(x), (0, 0, 3, 3, 3, 3))
    g = _f(dy)
    dw = torch.stack([torch.stack([(g * xp[:, kh:kh + H, kw:kw + W]).sum((0, 1, 2))
                                   for kw in range(7)], -1) for kh in range(7)], -2)
    return dw.reshape(C, 1, 7, 7), g.reshape(-1, C).sum(0)


def drop_path_keep(n: int, p: float, seed: int, device="cpu") -> Tensor:
    """[n] keep mask of stochastic depth in "row" mode: the dropout hash (:func:`dropout_keep`)
    applied to the sample index, so it depends only on (seed, sample)."""
    if p <= 0.0:
        return torch.ones(n, dtype=torch.bool, device=device)
    return dropout_keep(n, p, seed, device)


def _path_scale(f: Tensor, hw: int, p: float, seed: int) -> Tensor:
    """s_n per row [R, 1]: fp32(1 / (1 - p)) where sample n = r / hw is kept, else 0 (p == 0: 1)."""
    C = f.shape[-1]
    n = f.numel() // C // hw
    dt = torch.float64 if f.dtype == torch.float64 else torch.float32
    if p <= 0.0:
        return torch.ones(n * hw, 1, dtype=dt, device=f.device)
    inv = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).to(dt)
    s = drop_path_keep(n, p, seed, f.device).to(dt) * inv.to(f.device)
    return s.repeat_interleave(hw).reshape(-1, 1)


def scale_residual_fwd(f: Tensor, res: Tensor, gamma: Tensor, hw: int, p: float = 0.0,
                       seed: int = 0) -> Tensor:
    """out = T(fp32(res) + (fp32(f) * gamma[c]) * s_n): layer scale, stochastic depth by sample
    (rows r of sample n = r / hw) and the residual add in three rounded fp32 operations."""
    C = f.shape[-1]
    s = _path_scale(f, hw, p, seed)
    out = _f(res).reshape(-1, C) + (_f(f).reshape(-1, C) * _f(gamma).reshape(1, C)) * s
    return out.reshape(f.shape).to(f.dtype)


def scale_residual_bwd(dout: Tensor, f: Tensor, gamma: Tensor, hw: int, p: float = 0.0,
                       seed: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """(df, dgamma, dbias): df = T((fp32(dout) * gamma[c]) * s_n), dgamma[c] = sum_r (fp32(dout) *
    fp32(f)) * s_n, dbias[c] = sum_r fp32(df) (the stored, rounded values: the bias gradient of
    the Linear that produced f).  The residual's gradient is dout itself."""
    C = f.shape[-1]
    s = _path_scale(f, hw, p, seed)
    d = _f(dout).reshape(-1, C)
    df = ((d * _f(gamma).reshape(1, C)) * s).to(f.dtype)
    dgamma = ((d * _f(f).reshape(-1, C)) * s).sum(0)
    return df.reshape(f.shape), dgamma, _f(df).sum(0)


# ----------------------------------------------------------------------------- se.hip
def _cd(t: Tensor) -> torch.dtype:
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _const(v: float, like: Tensor) -> Tensor:
    """A 0-dim constant on ``like``'s device: dividing by it is a true division on every backend
    (a Python scalar divisor may become a multiplication by its reciprocal)."""
    return torch.full((), v, dtype=like.dtype, device=like.device)


def _recip(n: int, like: Tensor) -> Tensor:
    """fp32(1 / n) (the double quotient rounded once), as the launchers compute it; the double
    itself for float64 operands."""
    return torch.tensor(1.0 / n, dtype=like.dtype).to(like.device)


def _se_pre(y: Tensor, scale: Tensor, bias: Tensor) -> Tensor:
    """u = (fp32(y) * scale[c]) + bias[c]: two rounded operations."""
    dt = _cd(y)
    return (_f(y) * scale.to(dt)) + bias.to(dt)


def se_act(u: Tensor, act: str) -> Tensor:
    """relu: max(u, 0); hardswish: (u * clamp(u + 3, 0, 6)) / 6 with a true division."""
    if act == "relu":
        return torch.relu(u)
    if act == "hardswish":
        return (u * (u + 3.0).clamp(0.0, 6.0)) / _const(6.0, u)
    raise ValueError(f"bn_act_pool: act must be relu or hardswish, got {act!r}")


def se_act_grad(u: Tensor, e: Tensor, act: str) -> Tensor:
    """e * act'(u) by torch's rules at the knees (what ATen's backward kernels return).  relu:
    u > 0.  hardswish: 0 for u <= -3, e * ((u / 3) + 0.5) for -3 < u < 3, e for u >= 3."""
    zero = torch.zeros_like(e)
    if act == "relu":
        return torch.where(u > 0, e, zero)
    if act == "hardswish":
        mid = e * ((u / _const(3.0, u)) + 0.5)
        return torch.where(u <= -3.0, zero, torch.where(u < 3.0, mid, e))
    raise ValueError(f"bn_act_pool: act must be relu or hardswish, got {act!r}")


def hardsigmoid(gate: Tensor) -> Tensor:
    """s = clamp(fp32(gate) + 3, 0, 6) / 6."""
    g = _f(gate)
    return (g + 3.0).clamp(0.0, 6.0) / _const(6.0, g)


def bn_act_pool_fwd(y: Tensor, scale: Tensor, bias: Tensor, act: str,
                    want_pool: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """(z, pm): z = T(act(u)); pm [N, C] = (sum_hw fp32(z)) * (1 / HW) of the STORED z (what a
    separate pool would have read), or None."""
    N, H, W, C = y.shape
    z = se_act(_se_pre(y, scale, bias), act).to(y.dtype)
    if not want_pool:
        return z, None
    zf = _f(z)
    return z, zf.reshape(N, H * W, C).sum(1) * _recip(H * W, zf)


def _se_g(dz: Tensor, y: Tensor, scale: Tensor, bias: Tensor, act: str,
          dpm: Optional[Tensor]) -> Tensor:
    """g = e * act'(u), e = fp32(dz) + dpm[n, c] * (1 / HW) (the global pool's backward)."""
    N, H, W, C = y.shape
    e = _f(dz)
    if dpm is not None:
        e = e + (dpm.to(e.dtype).reshape(N, 1, 1, C) * _recip(H * W, e))
    return se_act_grad(_se_pre(y, scale, bias), e, act)


def bn_act_pool_bwd_reduce(dz: Tensor, y: Tensor, scale: Tensor, bias: Tensor, mean: Tensor,
                           invstd: Tensor, act: str,
                           dpm: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(sum g, sum g * xhat) per channel, xhat = (fp32(y) - mean[c]) * invstd[c]."""
    C = y.shape[-1]
    g = _se_g(dz, y, scale, bias, act, dpm)
    xhat = (_f(y) - mean.to(g.dtype)) * invstd.to(g.dtype)
    return g.reshape(-1, C).sum(0), (g * xhat).reshape(-1, C).sum(0)


def bn_act_pool_bwd_apply(dz: Tensor, y: Tensor, scale: Tensor, bias: Tensor, mean: Tensor,
                          invstd: Tensor, gamma: Tensor, act: str, dpm: Optional[Tensor] = None,
                          sum_g: Optional[Tensor] = None,
                          sum_gx: Optional[Tensor] = None) -> Tensor:
    """dy = T((gamma * invstd) * ((g - sum_g * (1 / cnt)) - xhat * (sum_gx * (1 / cnt)))), cnt =
    N * HW; without sums (eval-mode BN) dy = T((gamma * invstd) * g)."""
    C = y.shape[-1]
    g = _se_g(dz, y, scale, bias, act, dpm)
    k = gamma.to(g.dtype) * invstd.to(g.dtype)
    if sum_g is None:
        return (k * g).to(dz.dtype)
    inv = _recip(y.numel() // C, g)
    xhat = (_f(y) - mean.to(g.dtype)) * invstd.to(g.dtype)
    return (k * ((g - sum_g.to(g.dtype) * inv) - xhat * (sum_gx.to(g.dtype) * inv))).to(dz.dtype)


def se_scale_fwd(z: Tensor, gate: Tensor) -> Tensor:
    """out = T(fp32(z) * s), s = hardsigmoid(gate[n, c]); gate [N, C] or [N, 1, 1, C]."""
    N, H, W, C = z.shape
    return (_f(z) * hardsigmoid(gate).reshape(N, 1, 1, C)).to(z.dtype)


def se_scale_bwd(dout: Tensor, z: Tensor, gate: Tensor) -> Tuple[Tensor, Tensor]:
    """(dz, dgate): dz = T(fp32(dout) * s); dgate = T(q * s'), q[n, c] = sum_hw fp32(dout) *
    fp32(z), s' = fp32(1 / 6) for -3 < gate < 3, else 0."""
    N, H, W, C = z.shape
    d = _f(dout)
    dz = (d * hardsigmoid(gate).reshape(N, 1, 1, C)).to(z.dtype)
    q = (d * _f(z)).reshape(N, H * W, C).sum(1)
    gf = _f(gate).reshape(N, C)
    # fp32(1 / 6) in every precision, as the kernel's constant and ATen's hardsigmoid backward
    sixth = torch.tensor(1.0 / 6.0, dtype=torch.float32).to(device=gf.device, dtype=gf.dtype)
    sp = torch.where((gf > -3.0) & (gf < 3.0), sixth, torch.zeros_like(sixth))
    return dz, (q * sp).reshape(gate.shape).to(gate.dtype)
