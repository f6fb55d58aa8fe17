"""The depthwise K x K kernels of csrc/kernels/dwconvk.hip (K in {3, 5}, stride 1 / 2) against a
float64 ``F.conv2d(groups=C)`` and its autograd gradients.

Exact cases use small integers: with x in [-2, 2] and w in [-1, 1] an output is at most 50 in
magnitude and dx at most 52 (addend), exact in bf16 whatever the summation order.  The statistics
(v = y - shift, |shift| <= 1) and the weight-grad sums (|dy * x| <= 4) are exact in fp32 while the
sum of their magnitudes stays below 2^24; the large cases draw x from [-1, 1] to stay there, and
every case asserts these bounds on the reference.  (With pad (K - 1) / 2 every input row is reached
by a tap even where (H + 2p - K) % 2 = 1; the even maps are in the list all the same.)
"""
import pytest
import torch
import torch.nn.functional as F

from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu

dev = "cuda"
bf16 = torch.bfloat16
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
DTYPES = [bf16, torch.float32]
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


def ints(lo, hi, *shape, dtype=torch.float32):
    return torch.randint(lo, hi + 1, shape, device=dev).to(dtype)


def within(got, ref, n_terms, s_abs, dtype):
    """test_convnext_kernels_gpu.py's bound: |got - ref| <= 2 (n + 1) 2^-24 S + half ulp |ref|."""
    half = 2.0 ** -8 if dtype == bf16 else 2.0 ** -24
    bound = 2.0 * (n_terms + 1) * 2.0 ** -24 * s_abs + half * (ref.abs() + 2.0 ** -24 * s_abs)
    err = (d(got) - ref).abs()
    assert bool((err <= bound + 1e-300).all()), float((err - bound).max())


def reference(x, w, s, dy):
    """float64 (y, dx, dw) of the depthwise conv; x / dy NHWC, w [C, K, K, 1]."""
    k, C = w.shape[1], x.shape[-1]
    xr = d(x).permute(0, 3, 1, 2).requires_grad_(True)
    wr = d(w).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride=s, padding=(k - 1) // 2, groups=C)
    dx, dw = torch.autograd.grad(y, (xr, wr), d(dy).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous(), dw


def maps(k, s):
    """Input maps: 1x1, W < K, outputs of tile-1 / tile / tile+1 in each axis, two tiles plus one,
    odd maps (7 -> 4, 15 -> 8 under stride 2) and even ones ((H + 2p - K) % 2 = 1)."""
    C = native()
    th, tw, dt = C.dwk_tile_h(k, s), C.dwk_tile_w(k, s), C.DWK_DGRAD_TILE

    def inp(o):
        return (o - 1) * s + 1
    return [(1, 1), (4, 2), (inp(th - 1), inp(tw + 1)), (inp(th), inp(tw)), (inp(th + 1), inp(tw - 1)),
            (inp(2 * th + 1), inp(2 * tw + 1)), (7, 15), (15, 7), (8, 10), (dt + 1, 2 * dt + 2)]


def run_exact(k, s, dtype, N, H, W, C, xhi=2):
    x, w = ints(-xhi, xhi, N, H, W, C, dtype=dtype), ints(-1, 1, C, k, k, 1, dtype=dtype)
    shift = ints(-1, 1, C)
    y, ps, pss = K.dwconvk_fwd(x, w, s, shift)
    dy = ints(-2, 2, *y.shape, dtype=dtype)
    add = ints(-2, 2, N, H, W, C, dtype=dtype)
    ry, rdx, rdw = reference(x, w, s, dy)
    v = ry.reshape(-1, C) - d(shift)
    # the arithmetic of the module docstring, on the reference
    assert ry.abs().max() <= 256 and (rdx.abs().max() + 2) <= 256
    assert (v * v).sum(0).max() < EXACT and v.abs().sum(0).max() < EXACT
    assert 2.0 * xhi * dy.numel() / C < EXACT  # the weight-grad's sum of |dy * x| per tap
    assert y.dtype == dtype and torch.equal(d(y), ry)
    assert K.dwconvk_fwd(x, w, s)[1] is None and torch.equal(K.dwconvk_fwd(x, w, s)[0], y)
    assert torch.equal(d(ps), v.sum(0, keepdim=True)) and torch.equal(d(pss), (v * v).sum(0, keepdim=True))
    assert torch.equal(d(K.dwconvk_dgrad(dy, w, x.shape, s)), rdx)
    assert torch.equal(d(K.dwconvk_dgrad(dy, w, x.shape, s, add)), rdx + d(add))
    assert torch.equal(d(K.dwconvk_wgrad(dy, x, k, s)), rdw)
    tgt = ints(-3, 3, C * k * k)
    t0 = d(tgt)
    assert K.dwconvk_wgrad(dy, x, k, s, tgt) is None
    assert torch.equal(d(tgt), t0 + rdw.reshape(-1))


@pytest.mark.parametrize("mi", range(10))
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("k,s", KS)
def test_exact(k, s, dtype, mi):
    H, W = maps(k, s)[mi]
    cb = native().DWK_CHAN_BLOCK_F32 if dtype == torch.float32 else native().DWK_CHAN_BLOCK
    run_exact(k, s, dtype, 1 + 2 * (mi % 2), H, W, [8, 40, cb + 8, 3840][mi % 4])


@pytest.mark.parametrize("k,s,N,ho,wo", [(3, 1, 3, 10, 10), (5, 2, 3, 10, 10), (3, 2, 1, 46, 45),
                                         (5, 1, 1, 46, 45)],
                         ids=["rows>256-k3s1", "rows>256-k5s2", "grid-cap-k3s2", "grid-cap-k5s1"])
def test_exact_many_tiles(k, s, N, ho, wo):
    """300 output tiles: partial rows of the statistics and, at C = 8, of the weight-grad past
    256 (det_sum_rows' second level); 2070: past DWK_MAX_BLOCKS, a block walks several tiles."""
    C = native()
    H, W = (ho * C.dwk_tile_h(k, s) - 1) * s + 1, (wo * C.dwk_tile_w(k, s) - 1) * s + 1
    Ho, Wo = ho * C.dwk_tile_h(k, s), wo * C.dwk_tile_w(k, s)
    rows = C.dwk_stat_rows(N, Ho, Wo, k, s)
    assert rows == min(N * ho * wo, C.DWK_MAX_BLOCKS) > 256
    assert rows == C.DWK_MAX_BLOCKS or C.dwk_wgrad_rows(N, Ho, Wo, 8, k, s) == rows
    run_exact(k, s, bf16, N, H, W, 8, xhi=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("k,s", KS)
def test_random_and_relaunch(k, s, dtype):
    """Random operands within the per-element bound; pss, dx and dw bit-identical across two
    launches in default mode."""
    N, H, W, C = 2, 19, 37, 72
    x = torch.randn(N, H, W, C, device=dev).to(dtype)
    w = torch.randn(C, k, k, 1, device=dev).to(dtype)
    shift = torch.randn(C, device=dev)
    y, ps, pss = K.dwconvk_fwd(x, w, s, shift)
    dy = torch.randn(y.shape, device=dev).to(dtype)
    add = torch.randn(N, H, W, C, device=dev).to(dtype)
    ry, rdx, rdw = reference(x, w, s, dy)
    ay, adx, adw = reference(x.abs(), w.abs(), s, dy.abs())
    within(y, ry, k * k, ay, dtype)
    v = d(y).reshape(-1, C) - d(shift)
    n = v.shape[0]
    for got, term in ((ps, v), (pss, v * v)):
        within(got, term.sum(0, keepdim=True), n, term.abs().sum(0, keepdim=True), torch.float32)
    dx = K.dwconvk_dgrad(dy, w, x.shape, s, add)
    within(dx, rdx + d(add), k * k + 1, adx + d(add).abs(), dtype)
    dw = K.dwconvk_wgrad(dy, x, k, s)
    within(dw, rdw, n, adw, torch.float32)
    assert torch.equal(K.dwconvk_fwd(x, w, s, shift)[2], pss)
    assert torch.equal(K.dwconvk_dgrad(dy, w, x.shape, s, add), dx)
    assert torch.equal(K.dwconvk_wgrad(dy, x, k, s), dw)


def test_bad_arguments_raise():
    x, w = torch.randn(2, 9, 9, 16, device=dev).bfloat16(), torch.randn(16, 3, 3, 1, device=dev).bfloat16()
    y = K.dwconvk_fwd(x, w, 2)[0]
    sh = torch.zeros(16, device=dev)
    C = native()
    bad = [
        lambda: K.dwconvk_fwd(x, torch.zeros(16, 7, 7, 1, device=dev).bfloat16(), 1),  # K
        lambda: K.dwconvk_fwd(x, w, 3),                                                # stride
        lambda: K.dwconvk_fwd(x[..., :12].contiguous(), w[:12].contiguous(), 1),       # C % 8
        lambda: K.dwconvk_fwd(x, w.float(), 1),                                        # dtype
        lambda: K.dwconvk_fwd(x, w[:8].contiguous(), 1),                               # weight shape
        lambda: K.dwconvk_fwd(x, w, 1, sh[:8]),                                        # shift shape
        lambda: K.dwconvk_fwd(x, w, 1, torch.zeros(17, device=dev)[1:]),               # shift alignment
        lambda: K.dwconvk_fwd(torch.zeros(2 * 9 * 9 * 16 + 8, device=dev).bfloat16()[1:-7]
                              .reshape(2, 9, 9, 16), w, 1),                            # x alignment
        lambda: K.dwconvk_fwd(x[:0], w, 1),                                            # empty
        lambda: K.dwconvk_dgrad(y[:, :4].contiguous(), w, x.shape, 2),                 # dy vs Ho x Wo
        lambda: K.dwconvk_wgrad(y, x, 3, 1),                                           # dy vs Ho x Wo
        lambda: K.dwconvk_wgrad(y, x, 3, 2, torch.zeros(16 * 9 - 1, device=dev)),      # dw size
        lambda: C.dwconvk_dgrad(y, w, [2, 2 ** 14, 2 ** 14, 16], 2, None),             # >= 2^31
    ]
    for i, f in enumerate(bad):
        with pytest.raises((RuntimeError, ValueError, TypeError, NotImplementedError)):
            f()
            pytest.fail(f"bad call {i} did not raise")
    run_exact(3, 2, bf16, 2, 9, 9, 16)
