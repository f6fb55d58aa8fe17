"""The grouped 3 x 3 MFMA kernels of csrc/kernels/gconv3.hip (group width 8 ... 64, stride 1 / 2)
against a float64 ``F.conv2d(groups=...)`` and its autograd gradients.

Exact cases use small integers (x, dy in [-2, 2], w in [-1, 1]): every product and every partial
sum is an integer, so an fp32 sum is exact in any order while the sum of the terms' magnitudes
stays below 2^24 (asserted on the reference), and y / dx must equal the float64 result rounded
once to bf16.  The statistics are those of the rounded y (integers again).  (G, groups) covers a
full channel block plus a one-group tail (8 x 9, 16 x 5), output rows padded to 16 (24, 40) and
the largest weight image (64).
"""
import pytest
import torch
import torch.nn.functional as F

from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu

dev = "cuda"
bf16 = torch.bfloat16
WIDTHS = [(8, 9), (16, 5), (24, 3), (40, 2), (64, 1)]
EXACT = 2.0 ** 24


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(4242)
    yield


def d(t):
    return t.detach().double().cpu()


def ints(lo, hi, *shape, dtype=bf16):
    return torch.randint(lo, hi + 1, shape, device=dev).to(dtype)


def within(got, ref, n_terms, s_abs, dtype):
    """test_dwconvk_gpu.py's bound: |got - ref| <= 2 (n + 1) 2^-24 S + half ulp |ref|."""
    half = 2.0 ** -8 if dtype == bf16 else 2.0 ** -24
    bound = 2.0 * (n_terms + 1) * 2.0 ** -24 * s_abs + half * (ref.abs() + 2.0 ** -24 * s_abs)
    err = (d(got) - ref).abs()
    assert bool((err <= bound + 1e-300).all()), float((err - bound).max())


def reference(x, w, s, dy):
    """float64 (y, dx, dw [C, G, 3, 3]) of the grouped conv; x / dy NHWC, w [C, 3, 3, G]."""
    groups = x.shape[-1] // w.shape[-1]
    xr = d(x).permute(0, 3, 1, 2).requires_grad_(True)
    wr = d(w).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride=s, padding=1, groups=groups)
    dx, dw = torch.autograd.grad(y, (xr, wr), d(dy).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous(), dw


def maps(s):
    """Input maps: 1x1, narrower than the kernel, outputs of tile-1 / tile / tile+1 in each axis,
    two tiles plus one, odd and even maps under stride 2, the data-grad tile + 1."""
    C = native()
    th, tw, dt = C.gc3_tile_h(s), C.gc3_tile_w(s), C.GC3_DGRAD_TILE

    def inp(o):
        return (o - 1) * s + 1
    return [(1, 1), (4, 2), (inp(th - 1), inp(tw + 1)), (inp(th), inp(tw)), (inp(th + 1), inp(tw - 1)),
            (inp(2 * th + 1), inp(2 * tw + 1)), (7, 15), (15, 7), (8, 10), (dt + 1, 2 * dt + 2)]


def rounded(t):
    return t.float().to(bf16).double()


def run_exact(G, groups, s, N, H, W, xhi=2):
    C = G * groups
    x, w = ints(-xhi, xhi, N, H, W, C), ints(-1, 1, C, 3, 3, G)
    shift = ints(-1, 1, C, dtype=torch.float32)
    y, ps, pss = K.gconv3_fwd(x, w, s, shift)
    dy, add = ints(-2, 2, *y.shape), ints(-2, 2, N, H, W, C)
    ry, rdx, rdw = reference(x, w, s, dy)
    ay, adx, adw = reference(x.abs(), w.abs(), s, dy.abs())
    v = rounded(ry).reshape(-1, C) - d(shift)
    # the arithmetic of the module docstring, on the reference
    assert max(ay.max(), adx.max() + 2, adw.max()) < EXACT
    assert (v * v).sum(0).max() < EXACT and v.abs().sum(0).max() < EXACT
    assert y.dtype == bf16 and torch.equal(d(y), rounded(ry))
    assert K.gconv3_fwd(x, w, s)[1] is None and torch.equal(K.gconv3_fwd(x, w, s)[0], y)
    assert torch.equal(d(ps), v.sum(0, keepdim=True)) and torch.equal(d(pss), (v * v).sum(0, keepdim=True))
    assert torch.equal(d(K.gconv3_dgrad(dy, w, x.shape, s)), rounded(rdx))
    assert torch.equal(d(K.gconv3_dgrad(dy, w, x.shape, s, add)), rounded(rdx + d(add)))
    assert torch.equal(d(K.gconv3_wgrad(dy, x, G, s)), rdw)
    tgt = ints(-3, 3, C * G * 9, dtype=torch.float32)
    t0 = d(tgt)
    assert K.gconv3_wgrad(dy, x, G, s, tgt) is None
    assert torch.equal(d(tgt), t0 + rdw.reshape(-1))
    tgt = tgt.reshape(C, G, 3, 3).contiguous(memory_format=torch.channels_last)  # a parameter's view
    t0 = d(tgt)
    assert K.gconv3_wgrad(dy, x, G, s, tgt) is None and torch.equal(d(tgt), t0 + rdw)


@pytest.mark.parametrize("mi", range(10))
@pytest.mark.parametrize("G,groups", WIDTHS)
@pytest.mark.parametrize("s", [1, 2])
def test_exact(s, G, groups, mi):
    H, W = maps(s)[mi]
    run_exact(G, groups, s, 1 + 2 * (mi % 2), H, W)


@pytest.mark.parametrize("s,ho,wo", [(1, 46, 45), (2, 46, 45)], ids=["s1", "s2"])
def test_exact_many_tiles(s, ho, wo):
    """2070 output tiles: past GC3_MAX_BLOCKS (a block walks several tiles; at stride 2 the
    data-grad's tiles are past it too) and, with one channel block, 512 weight-grad slabs
    (det_sum_rows' second level)."""
    C = native()
    Ho, Wo = ho * C.gc3_tile_h(s), wo * C.gc3_tile_w(s)
    H, W = (Ho - 1) * s + 1, (Wo - 1) * s + 1
    assert C.gc3_stat_rows(1, Ho, Wo, s) == C.GC3_MAX_BLOCKS < ho * wo
    assert C.gc3_wgrad_rows(1, Ho, Wo, 8, 8, s) == C.GC3_WGRAD_MAX_ROWS > 256
    run_exact(8, 1, s, 1, H, W, xhi=1)


@pytest.mark.parametrize("G,groups", WIDTHS)
@pytest.mark.parametrize("s", [1, 2])
def test_random_and_relaunch(s, G, groups):
    """Random operands within the per-element summation bound; every entry bit-identical across
    two launches."""
    N, H, W, C = 2, 19, 37, G * groups
    x = torch.randn(N, H, W, C, device=dev).to(bf16)
    w = torch.randn(C, 3, 3, G, device=dev).to(bf16)
    shift = torch.randn(C, device=dev)
    y, ps, pss = K.gconv3_fwd(x, w, s, shift)
    dy = torch.randn(y.shape, device=dev).to(bf16)
    add = torch.randn(N, H, W, C, device=dev).to(bf16)
    ry, rdx, rdw = reference(x, w, s, dy)
    ay, adx, adw = reference(x.abs(), w.abs(), s, dy.abs())
    within(y, ry, 9 * G, ay, bf16)
    v = d(y).reshape(-1, C) - d(shift)
    n = v.shape[0]
    for got, term in ((ps, v), (pss, v * v)):
        within(got, term.sum(0, keepdim=True), n, term.abs().sum(0, keepdim=True), torch.float32)
    dx = K.gconv3_dgrad(dy, w, x.shape, s, add)
    within(dx, rdx + d(add), 9 * G + 1, adx + d(add).abs(), bf16)
    dw = K.gconv3_wgrad(dy, x, G, s)
    within(dw, rdw, n, adw, torch.float32)
    again = K.gconv3_fwd(x, w, s, shift)
    assert all(torch.equal(a, b) for a, b in zip(again, (y, ps, pss)))
    assert torch.equal(K.gconv3_dgrad(dy, w, x.shape, s, add), dx)
    assert torch.equal(K.gconv3_wgrad(dy, x, G, s), dw)


@pytest.mark.parametrize("G", [8, 24, 40])
@pytest.mark.parametrize("s", [1, 2])
def test_nan_stays_in_its_group_and_window(s, G):
    """One NaN pixel in the middle group of x (of dy): exactly the outputs whose window holds it
    are NaN.  K = 9 G (G, 2G, 4G in the stride-2 data-grad) is padded to 32: a padding k-slot that
    read an activation would carry the NaN into a neighbouring pixel or group."""
    N, H, W, C = 1, 11, 13, 3 * G
    x, w = ints(-2, 2, N, H, W, C), ints(-1, 1, C, 3, 3, G)
    w[w == 0] = 1
    x[0, 5, 6, G:2 * G] = float("nan")
    y = K.gconv3_fwd(x, w, s)[0]
    dy = ints(-2, 2, *y.shape)
    dy[0, 2, 3, G:2 * G] = float("nan")
    ry, rdx, _ = reference(x, w, s, dy)
    assert torch.equal(d(y).isnan(), ry.isnan()) and 0 < int(ry.isnan().sum()) <= 9 * G
    assert torch.equal(d(y).nan_to_num(0.5), rounded(ry).nan_to_num(0.5))
    dx = K.gconv3_dgrad(dy, w, x.shape, s)
    assert torch.equal(d(dx).isnan(), rdx.isnan()) and 0 < int(rdx.isnan().sum()) <= 9 * G


def test_bad_arguments_raise():
    x, w = torch.randn(2, 9, 9, 32, device=dev).bfloat16(), torch.randn(32, 3, 3, 16, device=dev).bfloat16()
    y = K.gconv3_fwd(x, w, 2)[0]
    sh = torch.zeros(32, device=dev)
    C = native()
    bad = [
        lambda: K.gconv3_fwd(x, torch.zeros(32, 5, 5, 16, device=dev).bfloat16(), 1),   # kernel size
        lambda: K.gconv3_fwd(x, w, 3),                                                  # stride
        lambda: K.gconv3_fwd(x, w[..., :12].contiguous(), 1),                           # G % 8
        lambda: K.gconv3_fwd(torch.zeros(1, 4, 4, 128, device=dev).bfloat16(),
                             torch.zeros(128, 3, 3, 128, device=dev).bfloat16(), 1),    # G > 64
        lambda: K.gconv3_fwd(x[..., :24].contiguous(), w[:24].contiguous(), 1),         # C % G
        lambda: K.gconv3_fwd(x.float(), w.float(), 1),                                  # dtype
        lambda: K.gconv3_fwd(x, w[:16].contiguous(), 1),                                # weight shape
        lambda: K.gconv3_fwd(x, w, 1, sh[:8]),                                          # shift shape
        lambda: K.gconv3_fwd(x, w, 1, torch.zeros(33, device=dev)[1:]),                 # shift alignment
        lambda: K.gconv3_fwd(torch.zeros(2 * 9 * 9 * 32 + 8, device=dev).bfloat16()[1:-7]
                             .reshape(2, 9, 9, 32), w, 1),                              # x alignment
        lambda: K.gconv3_fwd(x[:0], w, 1),                                              # empty
        lambda: K.gconv3_dgrad(y[:, :4].contiguous(), w, x.shape, 2),                   # dy vs Ho x Wo
        lambda: K.gconv3_wgrad(y, x, 16, 1),                                            # dy vs Ho x Wo
        lambda: K.gconv3_wgrad(y, x, 16, 2, torch.zeros(32 * 16 * 9 - 1, device=dev)),  # dw size
        lambda: C.gconv3_dgrad(y, w, [2, 2 ** 13, 2 ** 13, 32], 2, None),               # >= 2^31
    ]
    for i, f in enumerate(bad):
        with pytest.raises((RuntimeError, ValueError, TypeError, NotImplementedError)):
            f()
            pytest.fail(f"bad call {i} did not raise")
    run_exact(16, 2, 2, 2, 9, 9)
