"""The SiLU and sigmoid variants of se.hip against float64 on the inputs as stored.  They go through
expf, so they are not the bits of ops/_ref.py; ``test_ref_fp32_inside_the_bounds`` (CPU) holds
ops/_ref.py in the storage dtype to the same bounds on the same inputs, so the reference fixes
them, not the kernel.  E = 2^-24, T the output type's half ulp, u = y * scale + bias in fp32 (off
by <= 2 E A, A = |y * scale| + |bias|):

  z = u s(u):  |silu'| < 1.1 carries u's error, 2.2 E A; expf (<= 2 ulp), 1 + e, the division and
      the product <= 8 E |z| <= 8 E A.  Bound 2 T |ref| + 2^-20 A.  At u = -90, exp(90) = inf: s = 0.
  g = e s (1 + u (1 - s)):  |silu''| <= 0.5 carries E A |e|; six more operations <= 8.8 E |e|.
      Bound 2^-20 |e| (1 + A).
  dy = k ((g - mg) - xhat mgx), k = gamma invstd, M = |g| + |mg| + |xhat mgx|:
      2 T |ref| + 2^-20 |k| (|e| (1 + A) + M).
  sums: (n + k) E sum |term| as in test_se_kernels_gpu.py, plus the terms' own bounds above.
  out = z s(g), dz = dout s(g):  (2 T + 8 E) |ref|.
  dgate = q s (1 - s), q = sum dout z, Q = sum |dout z|:  the sum is off by (hw + 2) E Q with
      s' <= 1 / 4; s (1 - s) is off by <= 4 E absolutely (1 - s cancels near s = 1).
      Bound (hw + 2) E Q / 4 + 4 E Q + (2 T + 8 E) |ref|.
"""
import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available

bf16 = torch.bfloat16
E = 2.0 ** -24
T = {bf16: 2.0 ** -8, torch.float32: 2.0 ** -24}  # the output type's half ulp
# (N, H, W, C): C / 8 = 5 leaves idle threads; 33 x 33 cuts a sample into slices, the last one
# short; 300 samples of one slice each are 300 > 256 partial rows of the BatchNorm sums
SHAPES = [(2, 7, 7, 40), (1, 33, 33, 64), (300, 1, 2, 8)]


def dd(t):
    return t.detach().double().cpu()


def inputs(shape, dtype, dev):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    y = (2.0 * r(N, H, W, C)).to(dtype)
    scale, bias = 0.5 + r(C).abs(), r(C)
    scale[0], bias[0] = 1.0, 0.0
    flat = y.view(-1, C)
    flat[:4, 0] = torch.tensor([0.0, 20.0, -20.0, -90.0]).to(dtype)  # u = 0, |u| = 20, u = -90
    t = dict(y=y, scale=scale, bias=bias, mean=r(C), invstd=0.5 + r(C).abs(), gamma=r(C),
             dz=r(N, H, W, C).to(dtype), dpm=r(N, C), gate=(3.0 * r(N, C)).to(dtype),
             dout=r(N, H, W, C).to(dtype))
    t["gate"][0, 0] = -90.0
    return {k: v.to(dev) for k, v in t.items()}


def inside(got, ref, bound, what):
    err = (dd(got).reshape(ref.shape) - ref).abs()
    assert torch.isfinite(dd(got)).all(), what
    bound = bound + 2.0 ** -126  # below the smallest normal a result may be flushed to zero
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


def check(impl, t, dtype, pool):
    """``impl``: mipipe.ops.kernels on GPU tensors, or mipipe.ops._ref on CPU tensors."""
    c = {k: dd(v) for k, v in t.items()}
    N, H, W, C = c["y"].shape
    hw, n = H * W, N * H * W
    A = (c["y"] * c["scale"]).abs() + c["bias"].abs()
    z, pm = impl.bn_act_pool_fwd(t["y"], t["scale"], t["bias"], "silu", pool)
    rz, _ = _ref.bn_act_pool_fwd(c["y"], c["scale"], c["bias"], "silu", False)
    inside(z, rz, 2 * T[dtype] * rz.abs() + 2.0 ** -20 * A, "z")
    if pool:
        zs = dd(z).reshape(N, hw, C)
        inside(pm, zs.sum(1) / hw, (hw + 2) * E * zs.abs().sum(1) / hw, "pm")
    dpm = t["dpm"] if pool else None
    e = c["dz"] + (c["dpm"].reshape(N, 1, 1, C) / hw if pool else 0.0)
    rg = _ref._se_g(c["dz"], c["y"], c["scale"], c["bias"], "silu", c["dpm"] if pool else None)
    xh = (c["y"] - c["mean"]) * c["invstd"]
    eg = 2.0 ** -20 * e.abs() * (1 + A)
    sg, sgx = impl.bn_act_pool_bwd_reduce(t["dz"], t["y"], t["scale"], t["bias"], t["mean"],
                                          t["invstd"], "silu", dpm)
    for got, term, et, k, what in ((sg, rg, eg, 12, "sum g"),
                                   (sgx, rg * xh, eg * xh.abs() + 3 * E * (rg * xh).abs(), 15,
                                    "sum g xhat")):
        inside(got, term.sum((0, 1, 2)),
               (n + k) * E * term.abs().sum((0, 1, 2)) + et.sum((0, 1, 2)), what)
    dy = impl.bn_act_pool_bwd_apply(t["dz"], t["y"], t["scale"], t["bias"], t["mean"], t["invstd"],
                                    t["gamma"], "silu", dpm, sg, sgx)
    rdy = _ref.bn_act_pool_bwd_apply(c["dz"], c["y"], c["scale"], c["bias"], c["mean"],
                                     c["invstd"], c["gamma"], "silu", c["dpm"] if pool else None,
                                     dd(sg), dd(sgx))
    k = (c["gamma"] * c["invstd"]).abs()
    M = rg.abs() + dd(sg).abs() / n + (xh * dd(sgx)).abs() / n
    inside(dy, rdy, 2 * T[dtype] * rdy.abs() + 2.0 ** -20 * k * (e.abs() * (1 + A) + M), "dy")
    rel = 2 * T[dtype] + 8 * E
    out = impl.se_scale_fwd(t["dout"], t["gate"], "sigmoid")  # (any NHWC tensor serves as z)
    ro = _ref.se_scale_fwd(c["dout"], c["gate"], "sigmoid")
    inside(out, ro, rel * ro.abs(), "out")
    dz, dgate = impl.se_scale_bwd(t["dout"], z, t["gate"], "sigmoid")
    rdz, rdg = _ref.se_scale_bwd(c["dout"], dd(z), c["gate"], "sigmoid")
    inside(dz, rdz, rel * rdz.abs(), "dz")
    q_abs = (c["dout"] * dd(z)).abs().reshape(N, hw, C).sum(1)
    inside(dgate, rdg, (hw + 2) * E * q_abs / 4 + 4 * E * q_abs + rel * rdg.abs(), "dgate")


@pytest.mark.gpu
@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("dtype", [bf16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["idle", "slices", "rows300"])
def test_silu_sigmoid_kernels(shape, dtype, pool):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    N, H, W, C = shape
    sl = native().se_slices(N, H * W, C)
    assert [sl[0] * sl[1] < native().SE_THREADS, sl[3] > 1 and (H * W) % sl[2] != 0,
            N * sl[3] > 256][SHAPES.index(shape)]
    check(K, inputs(shape, dtype, "cuda"), dtype, pool)


@pytest.mark.parametrize("dtype", [bf16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["idle", "slices", "rows300"])
def test_ref_fp32_inside_the_bounds(shape, dtype):
    check(_ref, inputs(shape, dtype, "cpu"), dtype, True)
