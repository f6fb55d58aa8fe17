"""The squeeze-excitation / Hardswish kernels (csrc/kernels/se.hip) against their contracts in
mipipe.ops._ref.

Elementwise outputs (z, out, dz, and dy given the kernel's own sums) must equal the fp32 _ref,
evaluated on the CPU, bit for bit.  Sums are checked twice: exact-integer inputs (se_common),
where every order of summation gives the float64 result and ``torch.equal`` applies, at the slice
edges and past the grid caps derived from the module's SE_* constants; and random inputs against
float64 within (n + k) * 2^-24 * sum|term|, n the number of terms and k the rounded operations
that form one term (counted at each check below; the reference takes the branch and the slope's u
from the fp32 pre-activation of _ref, which the bit identity shows to be the kernel's own).
"""
import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops.determinism import deterministic
from mipipe.ops._native import native, native_available

import se_common as S

pytestmark = pytest.mark.gpu

dev = "cuda"
bf16 = torch.bfloat16
DTYPES = [bf16, torch.float32]
ACTS = ["relu", "hardswish"]
CHANNELS = [8, 16, 72, 88, 184, 960]
MAPS = [(1, 1, 1), (3, 1, 1), (2, 7, 7), (5, 5, 7), (2, 14, 14)]
EPS24 = 2.0 ** -24


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(777)
    yield


def consts():
    C = native()
    return {k: getattr(C, k) for k in S.SE_DEFAULTS}


def cpu(t):
    return None if t is None else t.detach().cpu()


def d(t):
    return None if t is None else t.detach().double().cpu()


def rand_case(N, H, W, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = dict(y=(r(N, H, W, C) * 3).to(dtype), scale=torch.rand(C, generator=g) + 0.5, bias=r(C),
             mean=r(C), invstd=torch.rand(C, generator=g) + 0.5, gamma=r(C), dz=r(N, H, W, C).to(dtype),
             dpm=r(N, C) * 4, dout=r(N, H, W, C).to(dtype), gate=(r(N, C) * 3).to(dtype))
    c["gate"].view(-1)[0::5] = 3.0   # the Hardsigmoid knees themselves
    c["gate"].view(-1)[1::7] = -3.0
    return c


def to_dev(c):
    return {k: (None if v is None else v.to(dev)) for k, v in c.items()}


def slice_edge_maps(C):
    """(N, H, W) around the slice rule for C channels, from the module's own geometry: one slice
    that is full / one row short, and two slices with a one-row last slice."""
    unit = S.se_unit_rows(C, consts())[1]
    return [(2, 1, hw) for hw in (unit, unit - 1, unit + 1, 2 * unit + 1) if hw >= 1]


def check_bits(N, H, W, C, dtype, act, seed=0, bounds=False):
    c = rand_case(N, H, W, C, dtype, seed)
    g = to_dev(c)
    bn = (g["scale"], g["bias"])
    st = (g["scale"], g["bias"], g["mean"], g["invstd"])
    cst = (c["scale"], c["bias"], c["mean"], c["invstd"])
    z, pm = K.bn_act_pool_fwd(g["y"], *bn, act, True)
    z_ref, _ = _ref.bn_act_pool_fwd(c["y"], c["scale"], c["bias"], act, False)
    assert torch.equal(cpu(z), z_ref), "z"
    z2, none = K.bn_act_pool_fwd(g["y"], *bn, act, False)
    assert none is None and torch.equal(z2, z), "pool=False"
    assert pm.dtype == torch.float32 and tuple(pm.shape) == (N, C)
    for dpm_on in (True, False):
        gd, cd = (g["dpm"], c["dpm"]) if dpm_on else (None, None)
        sg, sgx = K.bn_act_pool_bwd_reduce(g["dz"], g["y"], *st, act, gd)
        dy = K.bn_act_pool_bwd_apply(g["dz"], g["y"], *st, g["gamma"], act, gd, sg, sgx)
        dy_ref = _ref.bn_act_pool_bwd_apply(c["dz"], c["y"], *cst, c["gamma"], act, cd, cpu(sg),
                                            cpu(sgx))
        assert torch.equal(cpu(dy), dy_ref), f"dy (addend {dpm_on})"
        dye = K.bn_act_pool_bwd_apply(g["dz"], g["y"], *st, g["gamma"], act, gd)  # eval-mode BN
        dye_ref = _ref.bn_act_pool_bwd_apply(c["dz"], c["y"], *cst, c["gamma"], act, cd)
        assert torch.equal(cpu(dye), dye_ref), f"dy without sums (addend {dpm_on})"
        if bounds:
            check_bn_sums(c, act, cd, sg, sgx)
    for gate in (g["gate"], g["gate"].reshape(N, 1, 1, C)):
        out = K.se_scale_fwd(z, gate)
        assert torch.equal(cpu(out), _ref.se_scale_fwd(cpu(z), cpu(gate))), "out"
        dzs, dgate = K.se_scale_bwd(g["dout"], z, gate)
        dzs_ref, _ = _ref.se_scale_bwd(c["dout"], cpu(z), cpu(gate))
        assert torch.equal(cpu(dzs), dzs_ref), "dz of se_scale"
        assert dgate.shape == gate.shape and dgate.dtype == dtype
    if bounds:
        check_pool_sum(z, pm, H * W)
        check_gate_sum(c, z, dgate, H * W, dtype)


def _inside(got, ref, n, k, s_abs, what, extra=0.0):
    bound = (n + k) * EPS24 * s_abs + extra
    err = (d(got).reshape(ref.shape) - ref).abs()
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, bound min {float(bound.min()):.3e}, "
          f"worst err - bound {worst:.3e}")
    assert bool((err <= bound).all()), (what, worst)


def check_pool_sum(z, pm, hw):
    """pm = (sum of the stored z) * fp32(1 / HW).  A term is a stored value (no operation); the
    closing multiply is the one rounded operation besides the n - 1 additions: k = 1."""
    zf = d(z)
    N, C = zf.shape[0], zf.shape[-1]
    inv = float(torch.tensor(1.0 / hw, dtype=torch.float32))
    ref = zf.reshape(N, hw, C).sum(1) * inv
    _inside(pm, ref, hw, 1, zf.abs().reshape(N, hw, C).sum(1) * inv, "pm")


def check_gate_sum(c, z, dgate, hw, dtype):
    """dgate = T((sum dout * z) * s').  A term is one rounded product, the closing multiply one
    more: k = 2; T = bf16 then rounds the result once more (half an ulp: 2^-8 of it)."""
    zf, do = d(z), c["dout"].double()
    N, C = zf.shape[0], zf.shape[-1]
    gf = c["gate"].double()
    sp = ((gf > -3) & (gf < 3)).double() * float(torch.tensor(1.0 / 6.0, dtype=torch.float32))
    t = (do * zf).reshape(N, hw, C)
    ref = t.sum(1) * sp
    extra = ref.abs() * (2.0 ** -8 if dtype == bf16 else 0.0)
    _inside(dgate, ref, hw, 2, t.abs().sum(1) * sp, "dgate", extra)


def check_bn_sums(c, act, dpm, sg, sgx):
    """g = (dz + dpm * (1 / HW)) * ((u / 3) + 0.5): multiply, add, divide, add, multiply = 5
    rounded operations (ReLU and the no-addend form have fewer); g * xhat adds a subtraction and
    two multiplies, which the issue caps at k = 6."""
    y = c["y"]
    N, H, W, C = y.shape
    u = _ref._se_pre(y, c["scale"], c["bias"]).double()  # the fp32 pre-activation, as float64
    e = c["dz"].double()
    if dpm is not None:
        e = e + dpm.double().reshape(N, 1, 1, C) * float(torch.tensor(1.0 / (H * W),
                                                                      dtype=torch.float32))
    if act == "relu":
        gg = torch.where(u > 0, e, torch.zeros_like(e))
    else:
        gg = torch.where(u <= -3, torch.zeros_like(e), torch.where(u < 3, e * ((u / 3) + 0.5), e))
    xhat = (y.double() - c["mean"].double()) * c["invstd"].double()
    n = N * H * W
    _inside(sg, gg.sum((0, 1, 2)), n, 5, gg.abs().sum((0, 1, 2)), "sum g")
    _inside(sgx, (gg * xhat).sum((0, 1, 2)), n, 6, (gg * xhat).abs().sum((0, 1, 2)), "sum g xhat")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", CHANNELS)
def test_bit_identity(C, dtype):
    for i, (N, H, W) in enumerate(MAPS):
        for act in ACTS:
            check_bits(N, H, W, C, dtype, act, seed=C + i)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(1, 112, 112, 16), (2, 56, 56, 72)])
def test_bit_identity_long_maps(shape, dtype):
    """Several slices per sample with a short last slice (112^2 x 16), and exactly full ones."""
    N, H, W, C = shape
    sl = native().se_slices(N, H * W, C)
    assert sl[3] > 1
    for act in ACTS:
        check_bits(N, H, W, C, dtype, act, seed=5, bounds=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [8, 72, 960, 8 * 256 + 8])
def test_bit_identity_slice_edges(C, dtype):
    for i, (N, H, W) in enumerate(slice_edge_maps(C)):
        check_bits(N, H, W, C, dtype, ACTS[i % 2], seed=11 + i)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [16, 88, 960])
def test_random_sums_inside_the_bound(C, dtype):
    for i, (N, H, W) in enumerate([(2, 7, 7), (5, 5, 7), (2, 14, 14)]):
        for act in ACTS:
            check_bits(N, H, W, C, dtype, act, seed=100 + C + i, bounds=True)


def test_slice_rule_constants():
    """The exported rule is the one the tests derive their shapes from."""
    k = consts()
    for (N, HW, C) in [(2, 784, 72), (256, 49, 960), (1, 12544, 16), (4100, 1, 8)]:
        tpr, rpb, rows, slices, cy = native().se_slices(N, HW, C)
        assert (rpb, rpb * k["SE_ROW_U"]) == S.se_unit_rows(C, k)
        assert rows % (rpb * k["SE_ROW_U"]) == 0 and (slices - 1) * rows < HW <= slices * rows
        assert tpr * rpb <= k["SE_THREADS"] and cy == -(-(C // 8) // k["SE_THREADS"])


def _exact_shapes():
    return S.exact_shapes()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("act", ACTS)
def test_exact_sums(act, dtype):
    """Integer inputs: pm, q (through dgate), sum g and sum g xhat equal the float64 result, at the
    slice edges, past each grid cap and with the pooled-gradient addend on and off."""
    k = consts()
    shapes = S.exact_shapes(k)
    assert any(N > k["SE_MAX_BLOCKS"] for N, _, _, _ in shapes)
    assert any(N * H * W > k["SE_REDUCE_BLOCKS"] and H * W > 1 for N, H, W, _ in shapes)
    sixth = float(torch.tensor(1.0 / 6.0, dtype=torch.float32))
    for (N, H, W, C) in shapes:
        hw = H * W
        for with_dpm in ((True, False) if S.is_pow2(hw) else (False,)):
            c = S.exact_bn_case(N, H, W, C, seed=N + C + hw, with_dpm=with_dpm)
            z64, g64, gx64 = S.exact_bn_terms(c, act)
            S.assert_exact_terms(g64, 0.5, (0, 1, 2))
            S.assert_exact_terms(gx64, 0.25, (0, 1, 2))
            f = {n: (None if v is None else v.float().to(dev)) for n, v in c.items()}
            y, dz = f["y"].to(dtype), f["dz"].to(dtype)
            z, pm = K.bn_act_pool_fwd(y, f["scale"], f["bias"], act, True)
            assert torch.equal(d(z), z64), (N, H, W, C)
            inv = float(torch.tensor(1.0 / hw, dtype=torch.float32))
            assert torch.equal(cpu(pm), (z64.sum((1, 2)) * inv).float()), ("pm", N, H, W, C)
            sg, sgx = K.bn_act_pool_bwd_reduce(dz, y, f["scale"], f["bias"], f["mean"],
                                               f["invstd"], act, f["dpm"])
            assert torch.equal(d(sg), g64.sum((0, 1, 2))), ("sum g", N, H, W, C, with_dpm)
            assert torch.equal(d(sgx), gx64.sum((0, 1, 2))), ("sum g xhat", N, H, W, C, with_dpm)
        zz, dout, gate = S.exact_scale_case(N, H, W, C, seed=3 + N + C + hw)
        S.assert_exact_terms(dout * zz, 1.0, (1, 2))
        _, dgate = K.se_scale_bwd(dout.to(dev, dtype), zz.to(dev, dtype), gate.to(dev, dtype))
        sp = ((gate > -3) & (gate < 3)).double() * sixth
        assert torch.equal(cpu(dgate), ((dout * zz).sum((1, 2)) * sp).float().to(dtype)), \
            ("dgate", N, H, W, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_relaunch_is_bit_identical(dtype):
    N, H, W, C = 4, 14, 14, 184
    g = to_dev(rand_case(N, H, W, C, dtype, 9))
    st = (g["scale"], g["bias"], g["mean"], g["invstd"])

    def run():
        z, pm = K.bn_act_pool_fwd(g["y"], g["scale"], g["bias"], "hardswish", True)
        sg, sgx = K.bn_act_pool_bwd_reduce(g["dz"], g["y"], *st, "hardswish", g["dpm"])
        dy = K.bn_act_pool_bwd_apply(g["dz"], g["y"], *st, g["gamma"], "hardswish", g["dpm"], sg,
                                     sgx)
        out = K.se_scale_fwd(z, g["gate"])
        dzs, dgate = K.se_scale_bwd(g["dout"], z, g["gate"])
        return z, pm, sg, sgx, dy, out, dzs, dgate

    first = run()
    for mode in (False, True):
        with deterministic(mode):
            for a, b in zip(first, run()):
                assert torch.equal(a, b), mode


def test_bad_arguments_raise():
    g = to_dev(rand_case(2, 3, 3, 16, bf16, 1))
    y, sc, bi = g["y"], g["scale"], g["bias"]
    st = (sc, bi, g["mean"], g["invstd"])
    ok = K.bn_act_pool_fwd(y, sc, bi, "relu", True)[0]
    bad_c = torch.zeros(2, 3, 3, 12, device=dev, dtype=bf16)
    with pytest.raises(RuntimeError):      # C % 8 != 0
        K.bn_act_pool_fwd(bad_c, sc[:12].clone(), bi[:12].clone(), "relu", True)
    with pytest.raises(RuntimeError):      # the vectors do not match C
        K.bn_act_pool_fwd(y, sc[:8].clone(), bi, "relu")
    with pytest.raises(RuntimeError):      # mismatched shapes
        K.bn_act_pool_bwd_reduce(g["dz"][:1].contiguous(), y, *st, "relu")
    with pytest.raises(RuntimeError):      # dpm is not [N, C]
        K.bn_act_pool_bwd_reduce(g["dz"], y, *st, "relu", g["dpm"][:1].contiguous())
    with pytest.raises(RuntimeError):      # wrong dtype
        K.bn_act_pool_fwd(y.to(torch.float16), sc, bi, "relu")
    with pytest.raises(RuntimeError):
        K.bn_act_pool_bwd_apply(g["dz"].float(), y, *st, g["gamma"], "relu")
    with pytest.raises(RuntimeError):
        K.se_scale_fwd(ok, g["gate"].float())
    with pytest.raises(RuntimeError):      # empty input
        K.bn_act_pool_fwd(y[:0], sc, bi, "relu")
    with pytest.raises(RuntimeError):
        K.se_scale_fwd(ok[:0], g["gate"][:0])
    with pytest.raises(RuntimeError):      # gate of another batch size
        K.se_scale_bwd(g["dout"], ok, g["gate"][:1].contiguous())
    with pytest.raises(ValueError):        # an activation the kernels do not have
        K.bn_act_pool_fwd(y, sc, bi, "relu6")
    # a contiguous view that starts 2 bytes into an allocation
    flat = torch.zeros(y.numel() + 8, device=dev, dtype=bf16)
    mis = flat[1:1 + y.numel()].view(y.shape)
    assert mis.is_contiguous() and mis.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError):
        K.bn_act_pool_fwd(mis, sc, bi, "relu")
    with pytest.raises(RuntimeError):
        K.se_scale_fwd(mis, g["gate"])
    with pytest.raises(RuntimeError):
        K.se_scale_bwd(g["dout"], ok, flat[1:1 + 32].view(2, 16))
    vec = torch.zeros(20, device=dev)[1:17]
    with pytest.raises(RuntimeError):
        K.bn_act_pool_fwd(y, vec, bi, "relu")
    torch.cuda.synchronize()
