"""The MaxViT kernels on the GPU: relattn.hip's block / grid partition attention forward + backward
against the float64 reference of the bf16-rounded inputs (attention_common's per-slice measure and
tolerances: the arithmetic is the Swin kernel's plus one fp32 scale, so its bounds apply
unchanged), its exact properties and host checks; and se.hip's ``bn_act_pool(..., "gelu")``
against float64 within a derived bound.

GELU bound (E = 2^-24, T the output type's half ulp, u = y * scale + bias in fp32, off by <= 2 E A,
A = |y * scale| + |bias|).  The kernel's Φ is the one-exponential erfc expansion; evaluated in fp32
on the CPU over [-12, 12] (2e6 points + 5e5 normal draws) it is within 2.87e-7 = 2^-21.7 of
0.5 (1 + math.erf(u / √2)); with 1 E more for another expf it is below EPHI = 2^-21 = 8 E.
  z = u Φ(u):  |gelu'| < 1.13 carries u's error, 2.3 E A; Φ's error times |u| <= 8 E A; the
      product's rounding <= E A.  Bound 2 T |ref| + 2^-20 A.
  g = e (Φ + u φ):  |gelu''| <= 0.8 carries 1.6 E A |e|; Φ's error 8 E |e|; u φ, the sum and the
      product 3.3 E |e|.  Bound 2^-20 |e| (1 + A).
  dy and the sums: as test_se_silu_gpu.py derives them from g's bound.
"""
import functools

import pytest
import torch

import attention_common as AC
from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu
dev = "cuda"
D = 32
SCALE = 96 ** -0.5
DTABLE_TOL = AC.DQKV_TOL  # as test_swin_kernels_gpu.py: fp32 sums of fp32 dS
MODES = ("block", "grid")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"


def _past_caps():
    """One window more than a group of WIN_RUN, and more groups than WIN_MAX_RUNS slots."""
    C = native()
    return (C.WIN_RUN * C.WIN_MAX_RUNS + C.WIN_RUN + 1, 7, 7, 1)


CASES = {"one_window": (1, 7, 7, 1), "two_by_two": (2, 14, 14, 3), "non_square": (1, 14, 21, 2),
         "runs": (3, 28, 28, 2), "past_caps": _past_caps}


@functools.lru_cache(maxsize=None)
def case(name):
    """(shape, qkv, table, do) on the CPU; read-only."""
    shape = CASES[name]() if callable(CASES[name]) else CASES[name]
    B, Hs, Ws, H = shape
    g = torch.Generator().manual_seed(Hs * 100 + Ws * 10 + H)
    T = B * Hs * Ws
    qkv = (torch.randn(T, 3 * H * D, generator=g) * 1.5).to(torch.bfloat16)
    do = torch.randn(T, H * D, generator=g).to(torch.bfloat16)
    return shape, qkv, torch.randn(169, H, generator=g) * 0.5, do


@functools.lru_cache(maxsize=None)
def run(name, mode, scale=SCALE):
    shape, qkv, table, do = case(name)
    q, t, g = qkv.to(dev), table.to(dev), do.to(dev)
    o = K.partition_attention_fwd(q, t, *shape, mode, scale)
    return (o,) + tuple(K.partition_attention_bwd(g, q, t, *shape, mode, scale))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_partition_attention_against_float64(name, mode):
    (B, Hs, Ws, H), qkv, table, do = case(name)
    ro, rdqkv, rdt = _ref.partition_attention(qkv.double(), table.double(), B, Hs, Ws, H, mode,
                                              SCALE, do.double())
    o, dqkv, dtable = (t.cpu() for t in run(name, mode))
    S = Hs * Ws
    errs = {"O": AC.slice_err(o.reshape(B, S, H, D), ro.reshape(B, S, H, D),
                              AC.FLOOR_FRAC * float(ro.abs().max()))[0]}
    floor = AC.FLOOR_FRAC * float(rdqkv.abs().max())
    a, r = dqkv.reshape(B, S, 3, H, D), rdqkv.reshape(B, S, 3, H, D)
    for i, n in enumerate(("dQ", "dK", "dV")):
        errs[n] = AC.slice_err(a[:, :, i], r[:, :, i], floor)[0]
    errs["dtable"] = float((dtable.double() - rdt).abs().max() / rdt.abs().max())
    print(name, mode, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["O"] < AC.O_TOL
    assert max(errs["dQ"], errs["dK"], errs["dV"]) < AC.DQKV_TOL
    assert errs["dtable"] < DTABLE_TOL


def test_grid_equals_block_on_one_window():
    """Hs = Ws = 7: the grid stride is 1, the two partitions are the same."""
    for a, b in zip(run("one_window", "block"), run("one_window", "grid")):
        assert torch.equal(a, b)


def test_block_mode_equals_swin_kernel_at_its_scale():
    """Same operation order as winattn.hip at shift 0 (scale·log2e folded next to the bias add,
    no mask term): bit-equal outputs and gradients at scale 32^-1/2."""
    shape, qkv, table, do = case("two_by_two")
    q, t, g = qkv.to(dev), table.to(dev), do.to(dev)
    o, dqkv, dtable = run("two_by_two", "block", 32 ** -0.5)
    assert torch.equal(o, K.window_attention_fwd(q, t, *shape, 0))
    sq, st = K.window_attention_bwd(g, q, t, *shape, 0)
    assert torch.equal(dqkv, sq) and torch.equal(dtable, st)


@pytest.mark.parametrize("mode", MODES)
def test_backward_repeats_bit_for_bit(mode):
    shape, qkv, table, do = case("runs")
    args = (do.to(dev), qkv.to(dev), table.to(dev), *shape, mode, SCALE)
    for a, b in zip(run("runs", mode)[1:], K.partition_attention_bwd(*args)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("what,match", [("map", "7x7 partitions"), ("table", r"\[169, 1\]"),
                                        ("mode", "block")])
def test_argument_checks(what, match):
    t = torch.zeros(169, 1, device=dev)
    z = lambda r: torch.zeros(r, 96, dtype=torch.bfloat16, device=dev)  # noqa: E731
    with pytest.raises(RuntimeError, match=match):
        if what == "map":
            K.partition_attention_fwd(z(56), t, 1, 8, 7, 1, "block", SCALE)
        elif what == "table":
            K.partition_attention_fwd(z(49), t.reshape(-1), 1, 7, 7, 1, "grid", SCALE)
        else:
            K.partition_attention_fwd(z(49), t, 1, 7, 7, 1, "window", SCALE)


# ---- bn_act_pool(..., "gelu") -------------------------------------------------------------------
E = 2.0 ** -24
T = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
# (N, H, W, C): C / 8 = 5 (idle threads, below the 256-group block split); 33 x 33 cuts a sample
# into slices, the last one short; C / 8 = 257 takes a second block in grid.y
SHAPES = [(2, 7, 7, 40), (1, 33, 33, 64), (2, 3, 3, 2056)]


def dd(t):
    return t.detach().double().cpu()


def inside(got, ref, bound, what):
    err = (dd(got).reshape(ref.shape) - ref).abs()
    assert torch.isfinite(dd(got)).all(), what
    print(what, f"max err / bound = {float((err / (bound + 2.0 ** -126)).max()):.3f}")
    assert bool((err <= bound + 2.0 ** -126).all()), (what, float((err - bound).max()))


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["idle", "slices", "wide"])
def test_bn_gelu_pool_against_float64(shape, dtype, pool):
    N, H, W, C = shape
    sl = native().se_slices(N, H * W, C)
    assert [sl[0] * sl[1] < native().SE_THREADS, sl[3] > 1 and (H * W) % sl[2] != 0,
            sl[4] == 2][SHAPES.index(shape)]
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(y=(2.0 * r(N, H, W, C)).to(dtype), scale=0.5 + r(C).abs(), bias=r(C), mean=r(C),
             invstd=0.5 + r(C).abs(), gamma=r(C), dz=r(N, H, W, C).to(dtype), dpm=r(N, C))
    t["scale"][0], t["bias"][0] = 1.0, 0.0
    t["y"].view(-1, C)[:4, 0] = torch.tensor([0.0, 20.0, -20.0, -90.0]).to(dtype)
    c = {k: dd(v) for k, v in t.items()}
    t = {k: v.to(dev) for k, v in t.items()}
    hw, n = H * W, N * H * W
    A = (c["y"] * c["scale"]).abs() + c["bias"].abs()
    z, pm = K.bn_act_pool_fwd(t["y"], t["scale"], t["bias"], "gelu", pool)
    rz = torch.nn.functional.gelu(c["y"] * c["scale"] + c["bias"])
    inside(z, rz, 2 * T[dtype] * rz.abs() + 2.0 ** -20 * A, "z")
    if pool:
        zs = dd(z).reshape(N, hw, C)
        inside(pm, zs.sum(1) / hw, (hw + 2) * E * zs.abs().sum(1) / hw, "pm")
    dpm, cdpm = (t["dpm"], c["dpm"]) if pool else (None, None)
    e = c["dz"] + (c["dpm"].reshape(N, 1, 1, C) / hw if pool else 0.0)
    rg = _ref._se_g(c["dz"], c["y"], c["scale"], c["bias"], "gelu", cdpm)
    xh = (c["y"] - c["mean"]) * c["invstd"]
    eg = 2.0 ** -20 * e.abs() * (1 + A)
    stats = (t["scale"], t["bias"], t["mean"], t["invstd"])
    sg, sgx = K.bn_act_pool_bwd_reduce(t["dz"], t["y"], *stats, "gelu", dpm)
    for got, term, et, k, what in ((sg, rg, eg, 12, "sum g"),
                                   (sgx, rg * xh, eg * xh.abs() + 3 * E * (rg * xh).abs(), 15,
                                    "sum g xhat")):
        inside(got, term.sum((0, 1, 2)),
               (n + k) * E * term.abs().sum((0, 1, 2)) + et.sum((0, 1, 2)), what)
    dy = K.bn_act_pool_bwd_apply(t["dz"], t["y"], *stats, t["gamma"], "gelu", dpm, sg, sgx)
    rdy = _ref.bn_act_pool_bwd_apply(c["dz"], c["y"], c["scale"], c["bias"], c["mean"],
                                     c["invstd"], c["gamma"], "gelu", cdpm, dd(sg), dd(sgx))
    k = (c["gamma"] * c["invstd"]).abs()
    M = rg.abs() + dd(sg).abs() / n + (xh * dd(sgx)).abs() / n
    inside(dy, rdy, 2 * T[dtype] * rdy.abs() + 2.0 ** -20 * k * (e.abs() * (1 + A) + M), "dy")
