"""Shared inputs of the squeeze-excitation kernel tests (test_se_ref_cpu.py, test_se_kernels_gpu.py).

exact_bn_case / exact_scale_case build the exact-integer inputs: every term of every sum is a
multiple of a power-of-two quantum and the absolute terms add up to less than 2^24 quanta, so the
fp32 sum is exact in ANY order and must equal the float64 sum (assert_exact_terms checks that
premise on the terms themselves).
"""
import torch

# pre-activations u and what Hardswish makes of them: values {0, 0, 0, 3, 4, 6}, derivative
# factors {0, 0, 1/2, 1, 1, 1} (ATen's hardswish backward gives 0 at u = -3 and 1 at u = 3)
U_VALUES = (-5.0, -3.0, 0.0, 3.0, 4.0, 6.0)
HSWISH_OF_U = (0.0, 0.0, 0.0, 3.0, 4.0, 6.0)
HSWISH_SLOPE_OF_U = (0.0, 0.0, 0.5, 1.0, 1.0, 1.0)


def _pick(values, shape, gen):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def exact_bn_case(N, H, W, C, seed=0, with_dpm=True):
    """float64 tensors (cast them to the dtype under test: every value is a small dyadic number,
    exact in bf16): y, scale, bias, mean, invstd, gamma, dz, dpm, and the pre-activation u."""
    g = torch.Generator().manual_seed(seed)
    scale = _pick((0.5, 1.0), (C,), g)            # powers of two
    bias = _pick((-2.0, -1.0, 0.0, 1.0, 2.0), (C,), g)
    mean = _pick((-1.0, 0.0, 1.0), (C,), g)
    invstd = _pick((0.5, 1.0), (C,), g)
    gamma = _pick((0.5, 1.0, 2.0), (C,), g)
    u = _pick(U_VALUES, (N, H, W, C), g)
    y = (u - bias) / scale                        # integers, |y| <= 16
    dz = torch.randint(-4, 5, (N, H, W, C), generator=g).double()
    # dpm * (1 / HW) is a small integer: HW must be a power of two where dpm is used
    dpm = torch.randint(-3, 4, (N, C), generator=g).double() * (H * W) if with_dpm else None
    return dict(y=y, scale=scale, bias=bias, mean=mean, invstd=invstd, gamma=gamma, dz=dz,
                dpm=dpm, u=u)


def exact_bn_terms(c, act):
    """float64 (z, g, g * xhat) of an exact case, from the tables above (no formula of the code
    under test)."""
    u = c["y"] * c["scale"] + c["bias"]
    assert torch.equal(u, c["u"])
    z = torch.zeros_like(u)
    k = torch.zeros_like(u)
    for uv, zv, kv in zip(U_VALUES, HSWISH_OF_U, HSWISH_SLOPE_OF_U):
        m = u == uv
        z[m] = zv
        k[m] = kv if act == "hardswish" else float(uv > 0)
    N, H, W, C = u.shape
    e = c["dz"].clone()
    if c["dpm"] is not None:
        e = e + (c["dpm"] / (H * W)).reshape(N, 1, 1, C)
    gg = e * k
    xhat = (c["y"] - c["mean"]) * c["invstd"]
    return z, gg, gg * xhat


def exact_scale_case(N, H, W, C, seed=0):
    """float64 (z, dout, gate): integers in [0, 6] / [-4, 4]; gates on and beside the Hardsigmoid
    knees."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(0, 7, (N, H, W, C), generator=g).double()
    dout = torch.randint(-4, 5, (N, H, W, C), generator=g).double()
    gate = _pick((-4.0, -3.0, -1.5, 0.0, 1.5, 3.0, 4.0), (N, C), g)
    return z, dout, gate


def assert_exact_terms(terms, quantum, dims):
    """Every term is a multiple of ``quantum`` and, along ``dims``, the absolute terms add up to
    less than 2^24 quanta: every partial sum in every order is then a multiple of the quantum
    below 2^24 quanta, i.e. an fp32 number, and the fp32 sum equals the float64 sum."""
    t = terms.double() / quantum
    assert torch.equal(t, t.round()), "a term is not a multiple of the quantum"
    assert t.abs().sum(dims).max().item() < 2 ** 24, "the sum may leave fp32's exact range"


# se.hip's launch constants as this file was written; the GPU tests pass the built module's SE_*
# values instead, so the edge shapes follow the kernels
SE_DEFAULTS = dict(SE_THREADS=256, SE_ROW_U=4, SE_TARGET_BLOCKS=1024, SE_MAX_BLOCKS=4096,
                   SE_REDUCE_BLOCKS=1024)


def se_unit_rows(C, k=SE_DEFAULTS):
    """Rows a block takes per pass and per unrolled step: a slice is a multiple of the latter."""
    tpr = min(C // 8, k["SE_THREADS"])
    rpb = k["SE_THREADS"] // tpr
    return rpb, rpb * k["SE_ROW_U"]


def _hw(n):
    """(H, W) with H * W = n."""
    h = 1
    while h * h * 4 <= n and n % (h * 2) == 0:
        h *= 2
    return h, n // h


def exact_shapes(k=SE_DEFAULTS):
    """(N, H, W, C) of the exact-sum cases.  With few samples a slice is one unrolled step
    (unit rows), so HW = unit is one full slice, unit +- 1 a short slice / a one-row last slice and
    2 * unit two full slices; N > the grid caps makes blocks take several units; C > 8 * threads
    needs a second grid row."""
    out = []
    for C in (8, 72, 960):
        unit = se_unit_rows(C, k)[1]
        for hw in (unit, 2 * unit, unit + 1, unit - 1, max(1, unit // 2)):
            if hw >= 1:
                out.append((2,) + _hw(hw) + (C,))
    p2 = 1
    while p2 < se_unit_rows(72, k)[1]:
        p2 *= 2
    out.append((2,) + _hw(p2) + (72,))            # power-of-two HW with a short last slice
    out.append((2, 2, 2, 8 * k["SE_THREADS"] + 8))
    cap = max(k["SE_MAX_BLOCKS"], k["SE_REDUCE_BLOCKS"])
    out.append((cap + 4, 1, 1, 8))
    out.append((k["SE_REDUCE_BLOCKS"] + 6, 1, 2, 16))
    return sorted(set(out))


def is_pow2(n):
    return n & (n - 1) == 0
