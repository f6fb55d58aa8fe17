"""The fused data-grad epilogue's compile-time feature sets (csrc/kernels/epilogue.hpp EpiSet).

A bf16 data-grad whose fusion is exactly ADD (addend only), Y (BN reduce, mask recomputed from
y*scale + bias, no addend) or BITS_ADD (BN reduce, mask from the 1-bit copy, addend) runs a kernel
compiled for that set, on the tiles the training tuner picks for data-grads (0, 1, 9, 10, 14);
every other combination runs the run-time-generic epilogue.  Checked here:

* each set and its generic neighbours (bits without addend, z-mask + addend, Y + addend) on exact
  integer operands — dx, g, Σg and Σg·x̂ equal mipipe/ops/_ref.py bit for bit, in atomic and
  deterministic mode, over partial tiles, a full tile (the mask-free full-tile loop), BM - 1 rows,
  forward-style 3x3, stride-2 classes with the row remap and strided 1x1 with tap-less classes;
* the binding's report of the instantiation each launch took (dgrad_last_epi_sets): the three sets
  hit their kernels, the rest the generic one — a dispatch that always fell back would fail here;
* specialised vs forced-generic (generic_epi=True) on random bf16 data in deterministic mode:
  equal dx and equal slab rows.
"""
import pytest
import torch

from mipipe.ops import _ref, determinism
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu
dev = "cuda"

# tile id -> (BM, BN) (csrc/kernels/conv_common.hpp)
TILES = {0: (128, 128), 1: (128, 128), 9: (128, 64), 10: (64, 128), 14: (128, 128)}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(9731)
    yield


@pytest.fixture(params=[0, 1], ids=["atomic", "det"])
def det(request):
    old = determinism.deterministic_enabled()
    determinism.set_deterministic(bool(request.param))
    yield request.param
    determinism.set_deterministic(old)


def ints(lo, hi, *shape, dt=torch.bfloat16):
    return torch.randint(lo, hi + 1, shape, device=dev).to(dt)


def bn_vectors(Ci):
    mean = ints(-1, 1, Ci, dt=torch.float32)
    invstd = torch.tensor([0.5, 1.0, 2.0], device=dev)[torch.randint(0, 3, (Ci,), device=dev)]
    scale = torch.tensor([-1.0, 1.0, 2.0], device=dev)[torch.randint(0, 3, (Ci,), device=dev)]
    bias = ints(-1, 1, Ci, dt=torch.float32) + 0.5  # y*scale + bias is never 0
    return mean, invstd, scale, bias


def relu_bits(z, Ci):
    """(relu(z), its 1-bit mask) as bn_act_fwd(mask=) writes them."""
    bits = torch.empty(z.numel() // 8, dtype=torch.uint8, device=dev)
    zz = native().bn_act_fwd(z, torch.ones(Ci, device=dev), torch.zeros(Ci, device=dev), True,
                             None, None, None, bits)
    return zz, bits


# N, H, W, Ci, Co, k, s, p; "full" / "full-1": one dense tile of exactly BM (BM - 1) rows x BN columns
GEOMETRIES = [
    (1, 1, 129, 136, 64, 1, 1, 0),   # dense, tile + 1 rows, BN + 8 columns
    (3, 8, 8, 72, 64, 3, 1, 1),      # forward-style 3x3
    (2, 8, 8, 72, 64, 3, 2, 1),      # stride-2 parity classes: the row remap
    (2, 10, 10, 64, 128, 1, 2, 0),   # strided 1x1: classes without taps store the addend alone
    "full",
    "full-1",
]


def geometry(geo, cfg):
    BM, BN = TILES[cfg]
    if geo == "full":
        return (1, 1, BM, BN, 64, 1, 1, 0)
    if geo == "full-1":
        return (1, 1, BM - 1, BN, 64, 1, 1, 0)
    return geo


def took(want):
    sets = native().dgrad_last_epi_sets()
    assert len(sets) > 0 and all(s == want for s in sets), (want, sets)


def check_sums(rep, g, y, mean, invstd, Ci):
    sg, sgx = native().bn_bwd_collect(rep, Ci)
    gf = g.float().reshape(-1, Ci)
    xh = ((y.float() - mean) * invstd).reshape(-1, Ci)
    assert torch.equal(sg, gf.sum(0)) and torch.equal(sgx, (gf * xh).sum(0))
    assert float(rep.abs().max()) == 0.0


@pytest.mark.parametrize("cfg", sorted(TILES))
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: g if isinstance(g, str) else "x".join(map(str, g)))
def test_sets_and_generic_neighbours(geo, cfg, det):
    N, H, W, Ci, Co, k, s, p = geometry(geo, cfg)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = ints(-1, 1, N, Ho, Wo, Co)
    w = ints(-1, 1, Co, k, k, Ci)
    xs = [N, H, W, Ci]
    # the true result is an integer: rounding takes a transformed-domain reference algorithm's
    # last-bit noise out of the reference
    dxr = _ref.conv_dgrad(dy.float(), w.float(), tuple(xs), s, p).round()
    add = ints(-3, 3, N, H, W, Ci)
    assert float(dxr.abs().max()) + 3 <= 256  # integers a bf16 holds exactly
    y = ints(-4, 4, N, H, W, Ci)
    z = ints(-2, 2, N, H, W, Ci)
    zz, bits = relu_bits(z, Ci)
    mean, invstd, scale, bias = bn_vectors(Ci)
    rep = torch.zeros(3, native().STAT_REPLICAS, Ci, device=dev)
    ymask = (y.float() * scale + bias) > 0
    dg = native().conv_dgrad
    # ADD
    g = dg(dy, w, xs, s, p, add, cfg=cfg)
    took("ADD")
    assert torch.equal(g.float(), dxr + add.float())
    # Y
    g = dg(dy, w, xs, s, p, None, y, mean, invstd, scale, bias, rep, cfg=cfg)
    took("Y")
    assert torch.equal(g.float(), dxr * ymask)
    check_sums(rep, g, y, mean, invstd, Ci)
    # BITS_ADD
    g = dg(dy, w, xs, s, p, add, y, mean, invstd, scale, bias, rep, cfg=cfg, bn_mask=bits)
    took("BITS_ADD")
    assert torch.equal(g.float(), (dxr + add.float()) * (zz.float() > 0))
    check_sums(rep, g, y, mean, invstd, Ci)
    # generic: bits without addend
    g = dg(dy, w, xs, s, p, None, y, mean, invstd, scale, bias, rep, cfg=cfg, bn_mask=bits)
    took("generic")
    assert torch.equal(g.float(), dxr * (zz.float() > 0))
    check_sums(rep, g, y, mean, invstd, Ci)
    # generic: z-mask + addend
    g = dg(dy, w, xs, s, p, add, y, mean, invstd, scale, bias, rep, z, cfg=cfg)
    took("generic")
    assert torch.equal(g.float(), (dxr + add.float()) * (z.float() > 0))
    check_sums(rep, g, y, mean, invstd, Ci)
    # generic: Y + addend
    g = dg(dy, w, xs, s, p, add, y, mean, invstd, scale, bias, rep, cfg=cfg)
    took("generic")
    assert torch.equal(g.float(), (dxr + add.float()) * ymask)
    check_sums(rep, g, y, mean, invstd, Ci)
    # plain (no fusion) and fp32 never take a set
    dg(dy, w, xs, s, p, cfg=cfg)
    took("generic")


def test_fp32_takes_the_generic_epilogue():
    N, H, W, Ci, Co = 1, 1, 65, 72, 64
    dy = ints(-1, 1, N, H, W, Co, dt=torch.float32)
    w = ints(-1, 1, Co, 1, 1, Ci, dt=torch.float32)
    add = ints(-3, 3, N, H, W, Ci, dt=torch.float32)
    g = native().conv_dgrad(dy, w, [N, H, W, Ci], 1, 0, add)
    took("generic")
    assert torch.equal(g, _ref.conv_dgrad(dy, w, (N, H, W, Ci), 1, 0).round() + add)


@pytest.mark.parametrize("cfg", sorted(TILES))
@pytest.mark.parametrize("geo", ["full", (1, 1, 129, 136, 64, 1, 1, 0)], ids=["full", "partial"])
def test_specialised_equals_forced_generic(geo, cfg):
    """Random bf16 data (inexact sums): in deterministic mode each set's kernel and the generic
    one return equal dx and equal slab rows — same per-element arithmetic, same order of sums."""
    old = determinism.deterministic_enabled()
    determinism.set_deterministic(True)
    try:
        N, H, W, Ci, Co, k, s, p = geometry(geo, cfg)
        xs = [N, H, W, Ci]
        bf = dict(device=dev, dtype=torch.bfloat16)
        dy, w = torch.randn(N, H, W, Co, **bf), torch.randn(Co, k, k, Ci, **bf)
        add, y = torch.randn(N, H, W, Ci, **bf), torch.randn(N, H, W, Ci, **bf)
        _, bits = relu_bits(torch.randn(N, H, W, Ci, **bf), Ci)
        mean, bias = torch.randn(Ci, device=dev), torch.randn(Ci, device=dev)
        invstd, scale = torch.rand(Ci, device=dev) + 0.5, torch.randn(Ci, device=dev)
        bn = (y, mean, invstd, scale, bias)
        R = native().STAT_REPLICAS
        for name, addend, mask in (("ADD", add, None), ("Y", None, None), ("BITS_ADD", add, bits)):
            out = []
            for generic in (False, True):
                rep = torch.zeros(3, R, Ci, device=dev)
                args = (addend,) if name == "ADD" else (addend, *bn, rep)
                dx = native().conv_dgrad(dy, w, xs, s, p, *args, cfg=cfg, bn_mask=mask,
                                         generic_epi=generic)
                took("generic" if generic else name)
                out.append((dx, rep))
            assert torch.equal(out[0][0], out[1][0]), name
            assert torch.equal(out[0][1], out[1][1]), name
            if name != "ADD":
                assert float(out[0][1].abs().max()) > 0.0
    finally:
        determinism.set_deterministic(old)
