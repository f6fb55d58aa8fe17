"""``batch_mix`` on the MI355X (csrc/kernels/mix.hip) against ``_ref.batch_mix``, bit for bit.

Outputs are compared as integer words (uint32 for fp32, int16 for bf16).  Shapes: the small
record shapes, an odd width without a 16-byte run (3,5,7) and a row wider than a wave whose byte
length is no multiple of 16 (3,3,130: pairs whose rows do not share one alignment go element by
element); batches 1, 2, 5 (odd: the middle sample is its own partner) and 8; in place and out of
place."""
import functools

import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops import kernels as K

pytestmark = pytest.mark.gpu

SHAPES = [(3, 8, 8), (1, 28, 28), (3, 32, 32), (3, 5, 7), (3, 3, 130)]
BATCHES = [1, 2, 5, 8]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(autouse=True)
def _native():
    from mipipe.ops._native import load_error, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"


def _words(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _cutmix(H, W, y0, y1, x0, x1):
    lam = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
    return [lam, 2, y0, y1, x0, x1, 0, 0]


def descriptors(H, W):
    """name -> descriptor: every mode and the box cases that change the kernel's path."""
    ya, yb = H // 3, max(H // 3 + 1, 2 * H // 3)  # interior rows (H >= 3)
    xa, xb = W // 3, max(W // 3 + 1, 2 * W // 3)
    ax0 = 8 if W > 16 else 0  # a multiple of 8 elements: 16-byte aligned in both types
    d = {
        "none": [1, 0, 0, 0, 0, 0, 0, 0],
        "mixup-0": [0, 1, 0, 0, 0, 0, 0, 0],
        "mixup-1": [1, 1, 0, 0, 0, 0, 0, 0],
        "mixup-0.3": [0.3, 1, 0, 0, 0, 0, 0, 0],
        "cut-empty": _cutmix(H, W, ya, ya, xa, xb),
        "cut-empty-cols": _cutmix(H, W, ya, yb, xa, xa),
        "cut-full": _cutmix(H, W, 0, H, 0, W),
        "cut-pixel": _cutmix(H, W, ya, ya + 1, xa, xa + 1),
        "cut-top": _cutmix(H, W, 0, yb, xa, xb),
        "cut-bottom": _cutmix(H, W, ya, H, xa, xb),
        "cut-left": _cutmix(H, W, ya, yb, 0, xb),
        "cut-right": _cutmix(H, W, ya, yb, xa, W),
        "cut-odd-x0-odd-width": _cutmix(H, W, ya, yb, 1, min(W, 1 + (3 if W < 16 else 13))),
        "cut-aligned-x0": _cutmix(H, W, 0, yb, ax0, ax0 + (5 if W < 16 else 13)),
    }
    for k, v in d.items():
        assert 0 <= v[2] <= v[3] <= H and 0 <= v[4] <= v[5] <= W, (k, v)
    assert (d["cut-odd-x0-odd-width"][5] - 1) % 2 == 1 and d["cut-aligned-x0"][5] % 8 != 0
    return d


@functools.lru_cache(maxsize=None)
def _input(shape, B, dtype):
    g = torch.Generator().manual_seed(sum(shape) * 31 + B)
    return torch.randn(B, *shape, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _expected(shape, B, dtype, name):
    """The reference on the CPU (ATen's separate fp32 multiply / multiply / add), computed once."""
    x = _input(shape, B, dtype)
    mix = torch.tensor(descriptors(shape[1], shape[2])[name], dtype=torch.float32)
    return _ref.batch_mix(x, mix)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_mix_bit_equal(shape, B, dtype):
    C, H, W = shape
    x_cpu = _input(shape, B, dtype)
    x = x_cpu.cuda()
    for name, desc in descriptors(H, W).items():
        mix = torch.tensor(desc, dtype=torch.float32, device="cuda")
        want = _expected(shape, B, dtype, name)
        # out of place: a new tensor, and a given one; x is not written
        got = K.batch_mix(x, mix)
        assert got.data_ptr() != x.data_ptr() and got.dtype == dtype and got.shape == x.shape
        assert torch.equal(_words(got.cpu()), _words(want)), (name, "new")
        dst = torch.full_like(x, 7.0)
        assert K.batch_mix(x, mix, out=dst).data_ptr() == dst.data_ptr()
        assert torch.equal(_words(dst.cpu()), _words(want)), (name, "out")
        assert torch.equal(_words(x.cpu()), _words(x_cpu)), (name, "input written")
        # in place
        xin = x.clone()
        assert K.batch_mix(xin, mix, out=xin).data_ptr() == xin.data_ptr()
        res = xin.cpu()
        assert torch.equal(_words(res), _words(want)), (name, "in place")
        if desc[1] == 0:
            assert torch.equal(_words(res), _words(x_cpu)), name
        if desc[1] == 2:  # outside the box nothing changes
            y0, y1, x0, x1 = (int(v) for v in desc[2:6])
            outside = torch.ones(H, W, dtype=torch.bool)
            outside[y0:y1, x0:x1] = False
            assert torch.equal(_words(res)[:, :, outside], _words(x_cpu)[:, :, outside]), name
        if B % 2:  # the self-paired sample keeps its bits in every mode
            assert torch.equal(_words(res)[B // 2], _words(x_cpu)[B // 2]), name


def test_descriptor_is_read_at_run_time():
    """The same call with the descriptor rewritten on the device in between gives the other
    result: nothing of the descriptor is baked into the launch."""
    shape, B = (3, 32, 32), 8
    x_cpu = _input(shape, B, torch.float32)
    x = x_cpu.cuda()
    descs = descriptors(32, 32)
    mix = torch.tensor(descs["mixup-0.3"], dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    K.batch_mix(x, mix, out=out)
    first = out.cpu()
    mix.copy_(torch.tensor(descs["cut-bottom"], dtype=torch.float32), non_blocking=True)
    K.batch_mix(x, mix, out=out)
    second = out.cpu()
    assert torch.equal(_words(first), _words(_expected(shape, B, torch.float32, "mixup-0.3")))
    assert torch.equal(_words(second), _words(_expected(shape, B, torch.float32, "cut-bottom")))
    assert not torch.equal(first, second)


def test_larger_batch_fills_the_capped_grid():
    """More work units than the grid cap (grid-stride loop) and a row of 224 columns."""
    x = torch.randn(40, 3, 56, 224, generator=torch.Generator().manual_seed(5)).bfloat16()
    for desc in ([0.3, 1, 0, 0, 0, 0, 0, 0], _cutmix(56, 224, 9, 40, 3, 150)):
        mix = torch.tensor(desc, dtype=torch.float32)
        want = _ref.batch_mix(x, mix)
        xin = x.cuda()
        K.batch_mix(xin, mix.cuda(), out=xin)
        assert torch.equal(_words(xin.cpu()), _words(want))
        assert torch.equal(_words(K.batch_mix(x.cuda(), mix.cuda()).cpu()), _words(want))


def test_bad_arguments_raise():
    x = torch.randn(4, 3, 8, 8, device="cuda")
    mix = torch.tensor([1.0, 0, 0, 0, 0, 0, 0, 0], device="cuda")
    with pytest.raises(RuntimeError):
        K.batch_mix(x, mix[:4].contiguous())
    with pytest.raises(RuntimeError):
        K.batch_mix(x, mix.double())
    with pytest.raises(RuntimeError):
        K.batch_mix(x, mix.cpu())
    with pytest.raises(RuntimeError):
        K.batch_mix(x, mix, out=torch.empty(4, 3, 8, 8, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        K.batch_mix(x, mix, out=torch.empty(4, 3, 8, 9, device="cuda"))
    with pytest.raises(RuntimeError):
        K.batch_mix(x.permute(0, 1, 3, 2), mix)
    with pytest.raises(RuntimeError):
        K.batch_mix(x.half(), mix)
