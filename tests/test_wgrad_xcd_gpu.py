"""Split-K weight-grad block placement (set_wgrad_xcd): the 1-D grid placed by splitk_block_map
(a k-slice's tiles on one XCD) against grid(tiles, splits), for the generic conv weight-grad, the
patch-resident 3x3 kernel and the GEMM weight-grad.

The placement moves blocks, not arithmetic: the split -> k-range assignment and the ordered slice
sum are the same, so workspace plans must be bit-identical between the two placements; atomic
plans are checked against the fp32 reference.  K = 4*24*24 = 2304 output pixels = 36 k-steps, so
the requested splits 7 / 8 / 9 / 16 run as 6 / 8 / 9 / 12 slices with an uneven or clamped last
one.  Run on an MI355X:  python -m pytest tests -m gpu
"""
import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu

dev = "cuda"
TOL_WGRAD = {torch.bfloat16: 5e-3, torch.float32: 1e-4}  # tests/test_kernels_gpu.py
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
SPLITS = (1, 3, 7, 8, 9, 16)
WS = 1024  # plan flag: per-split workspace slices + ordered sum


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(4321)
    old = native().get_wgrad_xcd()
    yield
    native().set_wgrad_xcd(old)


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def hi_ref(t):
    """float64 on the CPU for fp32 kernels, fp32 on the GPU for bf16 kernels."""
    return t.detach().double().cpu() if t.dtype in (torch.float32, torch.float64) else t.float()


def tiles_of(dt):
    return (0, 2, 8) if dt == torch.float32 else (0, 2, 9)  # test_conv_wgrad_workspace_plans' set


def with_knob(on, fn):
    native().set_wgrad_xcd(on)
    return fn()


def check_plans(dt, run, ref, base):
    """run(out, plan) accumulates the weight-grad into out.  Workspace plans: knob off == knob on
    bit for bit, reruns bit-identical, both within TOL_WGRAD of ref; atomic plans with the knob
    on within TOL_WGRAD (5e-3 for bf16) of ref."""
    tol = TOL_WGRAD[dt]

    def go(plan):
        out = base.clone()
        run(out, plan)
        return out

    for cfg in tiles_of(dt):
        for sp in SPLITS:
            plan = (cfg + 16 * sp) | WS
            off = with_knob(False, lambda: go(plan))
            on = with_knob(True, lambda: go(plan))
            on2 = go(plan)
            assert torch.equal(off, on), (cfg, sp)
            assert torch.equal(on, on2), (cfg, sp)
            err = rel_err(hi_ref(on) - hi_ref(base), ref)
            print(f"ws cfg={cfg} sp={sp} rel_err={err:.3e}")
            assert err < tol, (cfg, sp, err)
            atom = go(cfg + 16 * sp)  # knob on
            err = rel_err(hi_ref(atom) - hi_ref(base), ref)
            print(f"atomic cfg={cfg} sp={sp} rel_err={err:.3e}")
            assert err < tol, (cfg, sp, err)


CONV_SHAPES = [
    # N, H, W, Ci, Co, k, s, p
    (4, 24, 24, 64, 256, 1, 1, 0),    # 2 tiles (128x128): fewer than 8
    (4, 24, 24, 256, 136, 1, 1, 0),   # partial M tile
    (4, 24, 24, 640, 128, 1, 1, 0),   # 5 tiles: not a multiple of 8
    (4, 48, 48, 128, 128, 3, 2, 1),   # generic im2col path
    (4, 24, 24, 128, 128, 3, 1, 1),   # 3x3 stride 1 (explicit plans run the generic kernel)
    (4, 24, 24, 64, 64, 3, 1, 1),
]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@DTYPES
def test_conv_wgrad_placements(shape, dt):
    N, H, W, Ci, Co, k, s, p = shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    assert N * Ho * Wo == 2304
    dy = torch.randn(N, Ho, Wo, Co, device=dev).to(dt)
    x = torch.randn(N, H, W, Ci, device=dev).to(dt)
    ref = _ref.conv_wgrad(hi_ref(dy), hi_ref(x), k, k, s, p)
    base = torch.randn(ref.shape, device=dev)
    check_plans(dt, lambda out, plan: native().conv_wgrad(dy, x, k, k, s, p, out, cfg=plan),
                ref, base)


# the two 3x3 stride-1 shapes above (4 tiles / 1 tile of 64 co x 64 ci, 48 slices of one k-step)
# and one whose 275 k-steps split into 138 slices with a short last one
W3_SHAPES = [(4, 24, 24, 128, 128), (4, 24, 24, 64, 64), (25, 22, 24, 64, 64)]


@pytest.mark.parametrize("shape", W3_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad3x3_placements(shape):
    """The patch-resident 3x3 kernel (plan -1 routes bf16 3x3 / stride-1 shapes to it): always
    workspace slices + ordered sum, so both placements and reruns are bit-identical."""
    N, H, W, Ci, Co = shape
    assert native().get_wgrad3x3()
    dy = torch.randn(N, H, W, Co, device=dev).to(torch.bfloat16)
    x = torch.randn(N, H, W, Ci, device=dev).to(torch.bfloat16)
    ref = _ref.conv_wgrad(dy.float(), x.float(), 3, 3, 1, 1)
    base = torch.randn(ref.shape, device=dev)

    def go():
        out = base.clone()
        native().conv_wgrad(dy, x, 3, 3, 1, 1, out)
        return out

    off = with_knob(False, go)
    on = with_knob(True, go)
    on2 = go()
    assert torch.equal(off, on) and torch.equal(on, on2)
    err = rel_err(on - base, ref)
    print(f"wgrad3x3 {shape} rel_err={err:.3e}")
    assert err < TOL_WGRAD[torch.bfloat16]


@pytest.mark.parametrize("NK", [(768, 256), (72, 200)], ids=["768x256", "72x200"])
@DTYPES
def test_linear_wgrad_placements(NK, dt):
    """Linear weight-grad dW[N][K] += dy[M][N]^T x[M][K] over M = 2304 rows (gemm.hip, beta = 1)."""
    M = 2304
    N, K = NK
    dy = torch.randn(M, N, device=dev).to(dt)
    x = torch.randn(M, K, device=dev).to(dt)
    ref = hi_ref(dy).t() @ hi_ref(x)
    base = torch.randn(N, K, device=dev)
    check_plans(dt, lambda out, plan: native().gemm(dy, x, True, False, None, "none",
                                                    torch.float32, out, 1.0, plan=plan),
                ref, base)


COLLECT_CASES = [
    # shape, plan (-1: the 3x3 kernel for 3x3 stride-1 shapes)
    ((4, 24, 24, 640, 128, 1, 1, 0), (0 + 16 * 8) | WS),
    ((4, 24, 24, 640, 128, 1, 1, 0), 0 + 16 * 9),
    ((4, 24, 24, 64, 256, 1, 1, 0), (2 + 16 * 7) | WS),
    ((4, 48, 48, 128, 128, 3, 2, 1), (9 + 16 * 16) | WS),
    ((4, 24, 24, 128, 128, 3, 1, 1), -1),
]


@pytest.mark.parametrize("shape,plan", COLLECT_CASES)
def test_bn_collect_rider_runs_once(shape, plan):
    """The BN-backward collect riding in a weight-grad launch sums the replica rows of a slab,
    zeroes them and adds to dgamma / dbeta: run by exactly one block of either grid form, or the
    second run would collect the zeroed slab (outputs 0, accumulators unchanged)."""
    N, H, W, Ci, Co, k, s, p = shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(N, Ho, Wo, Co, device=dev).to(torch.bfloat16)
    x = torch.randn(N, H, W, Ci, device=dev).to(torch.bfloat16)
    R, C = native().STAT_REPLICAS, 200
    slab = torch.randn(3, R, C, device=dev)
    acc = torch.randn(2, C, device=dev)

    def go():
        rep = slab.clone()
        out = torch.full((2, C), float("nan"), device=dev)
        dgamma, dbeta = acc[0].clone(), acc[1].clone()
        native().conv_wgrad(dy, x, k, k, s, p, cfg=plan, col_rep=rep, col_out=out,
                            col_dgamma=dgamma, col_dbeta=dbeta)
        return rep, out, dgamma, dbeta

    off = with_knob(False, go)
    on = with_knob(True, go)
    for a, b in zip(off, on):
        assert torch.equal(a, b)
    rep, out, dgamma, dbeta = on
    assert float(rep[:2].abs().max()) == 0.0 and torch.equal(rep[2], slab[2])
    assert rel_err(out[0], slab[0].sum(0)) < 1e-5 and rel_err(out[1], slab[1].sum(0)) < 1e-5
    assert rel_err(dgamma - acc[0], slab[1].sum(0)) < 1e-5
    assert rel_err(dbeta - acc[1], slab[0].sum(0)) < 1e-5
