"""Conv / GEMM output epilogue at its tile edges, on exact integer-valued operands.

x, w, dy, the addend and the BN vectors are small integers (or powers of two), so y, dx, Σ(y-s),
Σ(y-s)², Σg and Σg·x̂ are exact in bf16 / fp32 whatever the summation order: the kernels must equal
the reference (mipipe/ops/_ref.py) bit for bit, in the default (float-atomic) and the deterministic
mode.  Rows: one full tile, tile ± 1 (the statistics' full-tile path beside the partial-tile
one); columns: 8, BN - 8, BN + 8; one and two k-steps; every 4-wave training tile and the 8-wave
14.

What the partial-tile cases can and cannot see: rows past M of a conv tile are staged as exact
zeros (zero-filled operands), and the binding refuses a bias or ReLU together with statistics, so
no caller can stage anything else there.  These cases therefore pin the row count n in
Σ(y-s) = Σy - n·s and Σ(y-s)² (the shift is non-zero in most columns) and the full / partial path
choice, not the row mask's own bits; a wrong mask that zeroes rows INSIDE M would still show.
"""
import pytest
import torch

from mipipe.ops import _ref, determinism
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu
dev = "cuda"

# tile id -> (BM, BN) (csrc/kernels/conv_common.hpp)
TILES = {0: (128, 128), 1: (128, 128), 2: (128, 64), 8: (64, 128), 9: (128, 64), 10: (64, 128),
         14: (128, 128)}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(4321)
    yield


@pytest.fixture(params=[0, 1], ids=["atomic", "det"])
def det(request):
    old = determinism.deterministic_enabled()
    determinism.set_deterministic(bool(request.param))
    yield request.param
    determinism.set_deterministic(old)


def ints(lo, hi, *shape, dt=torch.bfloat16):
    return torch.randint(lo, hi + 1, shape, device=dev).to(dt)


def check_fwd(x, w, s, p, cfg):
    Co = w.shape[0]
    shift = ints(-2, 2, Co, dt=torch.float32)
    y, ps, pss = native().conv_fwd(x, w, s, p, shift, cfg=cfg)
    # the true result is an integer: rounding takes a transformed-domain reference algorithm's
    # last-bit noise out of the reference
    yr = _ref.conv_fwd(x.float(), w.float(), s, p, shift)[0].round()
    assert float(yr.abs().max()) <= 256  # integers a bf16 holds exactly
    assert torch.equal(y.float(), yr)
    d = (yr - shift).double().reshape(-1, Co)
    assert torch.equal(ps.sum(0).double(), d.sum(0))
    assert torch.equal(pss.sum(0).double(), (d * d).sum(0))
    y2 = native().conv_fwd(x, w, s, p, None, cfg=cfg)[0]  # no statistics: same output
    assert torch.equal(y, y2)


@pytest.mark.parametrize("cfg", sorted(TILES))
def test_fwd_dense_tile_edges(cfg, det):
    BM, BN = TILES[cfg]
    for K in (64, 128):
        for M in (BM, BM + 1, BM - 1):
            for Co in (8, BN - 8, BN + 8):
                x = ints(-1, 1, 1, 1, M, K)
                w = ints(-1, 1, Co, 1, 1, K)
                check_fwd(x, w, 1, 0, cfg)


@pytest.mark.parametrize("cfg", sorted(TILES))
def test_fwd_3x3_tile_edges(cfg, det):
    BM, BN = TILES[cfg]
    for N in (BM // 64, BM // 64 + 1, 1):  # 8 x 8 outputs: full tiles, a partial one, half a tile
        for Co in (8, BN + 8):
            x = ints(-1, 1, N, 8, 8, 64)
            w = ints(-1, 1, Co, 3, 3, 64)
            w = w * (torch.rand_like(w.float()) < 0.5).to(w.dtype)  # |y| stays below 256
            check_fwd(x, w, 1, 1, cfg)


def bn_vectors(Ci):
    mean = ints(-1, 1, Ci, dt=torch.float32)
    invstd = torch.tensor([0.5, 1.0, 2.0], device=dev)[torch.randint(0, 3, (Ci,), device=dev)]
    scale = torch.tensor([-1.0, 1.0, 2.0], device=dev)[torch.randint(0, 3, (Ci,), device=dev)]
    bias = ints(-1, 1, Ci, dt=torch.float32) + 0.5  # y*scale + bias is never 0
    return mean, invstd, scale, bias


def check_sums(rep, g, y, mean, invstd, Ci):
    sg, sgx = native().bn_bwd_collect(rep, Ci)
    gf = g.float().reshape(-1, Ci)
    xh = ((y.float() - mean) * invstd).reshape(-1, Ci)
    assert torch.equal(sg, gf.sum(0)) and torch.equal(sgx, (gf * xh).sum(0))
    assert float(rep.abs().max()) == 0.0


DGRAD_CASES = [
    # N, H, W, Ci, Co, k, s, p
    (1, 1, 129, 136, 64, 1, 1, 0),   # dense, tile + 1 rows, BN + 8 columns
    (3, 8, 8, 72, 64, 3, 1, 1),      # forward-style 3x3
    (2, 8, 8, 72, 64, 3, 2, 1),      # stride-2 parity classes: the row remap
    (2, 10, 10, 64, 128, 1, 2, 0),   # strided 1x1: classes without taps store the addend alone
]


@pytest.mark.parametrize("cfg", [0, 1, 9, 10, 14])
@pytest.mark.parametrize("case", DGRAD_CASES)
def test_dgrad_fusions(case, cfg, det):
    """plain, + addend, + BN-backward reduce with the mask from y, + mask from z."""
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = ints(-1, 1, N, Ho, Wo, Co)
    w = ints(-1, 1, Co, k, k, Ci)
    xs = [N, H, W, Ci]
    dxr = _ref.conv_dgrad(dy.float(), w.float(), tuple(xs), s, p).round()  # (see check_fwd)
    add = ints(-3, 3, N, H, W, Ci)
    assert float(dxr.abs().max()) + 3 <= 256
    assert torch.equal(native().conv_dgrad(dy, w, xs, s, p, cfg=cfg).float(), dxr)
    assert torch.equal(native().conv_dgrad(dy, w, xs, s, p, add, cfg=cfg).float(), dxr + add.float())
    y = ints(-4, 4, N, H, W, Ci)
    mean, invstd, scale, bias = bn_vectors(Ci)
    R = native().STAT_REPLICAS
    rep = torch.zeros(3, R, Ci, device=dev)
    g = native().conv_dgrad(dy, w, xs, s, p, None, y, mean, invstd, scale, bias, rep, cfg=cfg)
    assert torch.equal(g.float(), dxr * ((y.float() * scale + bias) > 0))
    check_sums(rep, g, y, mean, invstd, Ci)
    z = ints(-2, 2, N, H, W, Ci)
    g = native().conv_dgrad(dy, w, xs, s, p, add, y, mean, invstd, scale, bias, rep, z, cfg=cfg)
    assert torch.equal(g.float(), (dxr + add.float()) * (z.float() > 0))
    check_sums(rep, g, y, mean, invstd, Ci)


@pytest.mark.parametrize("cfg", [1, 9])
def test_dgrad_two_branch(cfg, det):
    N, H, W, Ci, Co = 1, 1, 127, 72, 64
    dy = ints(-1, 1, N, H, W, Co)
    w = ints(-1, 1, Co, 1, 1, Ci)
    x = ints(-1, 1, N, H, W, Ci)
    add = ints(-3, 3, N, H, W, Ci)
    y, y2 = ints(-4, 4, N, H, W, Ci), ints(-4, 4, N, H, W, Ci)
    mean, invstd, scale, bias = bn_vectors(Ci)
    mean2, invstd2, _, _ = bn_vectors(Ci)
    z = ints(-2, 2, N, H, W, Ci)
    bits = torch.empty(z.numel() // 8, dtype=torch.uint8, device=dev)
    zz = native().bn_act_fwd(z, torch.ones(Ci, device=dev), torch.zeros(Ci, device=dev), True,
                             None, None, None, bits)
    rep = torch.zeros(3, native().STAT_REPLICAS, Ci, device=dev)
    g = native().conv_dgrad(dy, w, [N, H, W, Ci], 1, 0, add, y, mean, invstd, scale, bias, rep,
                            None, cfg=cfg, bn_mask=bits, bn_y2=y2, bn_mean2=mean2,
                            bn_invstd2=invstd2)
    out3 = torch.empty(3, Ci, device=dev)
    native().conv_wgrad(dy, x, 1, 1, 1, 0, col_rep=rep, col_out=out3, col_two=True)
    dxr = _ref.conv_dgrad(dy.float(), w.float(), (N, H, W, Ci), 1, 0).round() + add.float()
    assert torch.equal(g.float(), dxr * (zz.float() > 0))
    gf = g.float().reshape(-1, Ci)
    assert torch.equal(out3[0], gf.sum(0))
    assert torch.equal(out3[1], (gf * ((y.float() - mean) * invstd).reshape(-1, Ci)).sum(0))
    assert torch.equal(out3[2], (gf * ((y2.float() - mean2) * invstd2).reshape(-1, Ci)).sum(0))


@pytest.mark.parametrize("act", ["relu", "none"])
def test_gemm_dense_bias_act(act):
    """The dense GEMM's bias / ReLU epilogue on the heuristic plan (no tile is forced)."""
    M, N, K = 129, 136, 128
    a, b = ints(-1, 1, M, K), ints(-1, 1, N, K)
    bias = ints(-3, 3, N, dt=torch.float32)
    want = a.float() @ b.float().t()
    for bv in (bias, None):
        r = want + bias if bv is not None else want
        r = torch.relu(r) if act == "relu" else r
        out = native().gemm(a, b, False, True, bv, act, torch.bfloat16, None, 0.0)
        assert torch.equal(out.float(), r)
