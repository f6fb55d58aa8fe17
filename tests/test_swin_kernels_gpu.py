"""The Swin kernels (csrc/kernels/winattn.hip) on the GPU: window attention forward + backward
against the float64 reference of the bf16-rounded inputs (attention_common's per-slice measure and
tolerances), its exact properties, patch_merge bit for bit, and the host argument checks."""
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
# dtable: the kernel sums fp32 dS (never rounded to bf16) in fp32, so the attention gradients'
# tolerance, relative to the largest |ref dtable|, has ample room
DTABLE_TOL = AC.DQKV_TOL


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"


def _past_caps():
    """One window more than a group of WIN_RUN, and more groups than WIN_MAX_RUNS slots: the
    partial last group (idle waves) and the grid stride.  One 7x7 window per sample."""
    C = native()
    return (C.WIN_RUN * C.WIN_MAX_RUNS + C.WIN_RUN + 1, 7, 7, 1, (3, 3))


CASES = {"one_window": (1, 7, 7, 1, (0, 0)), "all_regions": (2, 14, 14, 3, (3, 3)),
         "non_square": (1, 14, 21, 2, (3, 3)), "single_window_axis": (1, 7, 14, 2, (0, 3)),
         "past_caps": _past_caps}


@functools.lru_cache(maxsize=None)
def case(name):
    """(shape, qkv, table, do on the CPU, float64 reference (o, dqkv, dtable)); read-only."""
    shape = CASES[name]() if callable(CASES[name]) else CASES[name]
    B, Hs, Ws, H, shift = shape
    g = torch.Generator().manual_seed(Hs * 100 + Ws * 10 + H)
    T = B * Hs * Ws
    qkv = (torch.randn(T, 3 * H * D, generator=g) * 1.5).to(torch.bfloat16)
    do = torch.randn(T, H * D, generator=g).to(torch.bfloat16)
    table = torch.randn(169, H, generator=g) * 0.5
    ref = _ref.window_attention(qkv.double(), table.double(), B, Hs, Ws, H, shift, do.double())
    return shape, qkv, table, do, ref


def run(name):
    shape, qkv, table, do, ref = case(name)
    q, t, g = qkv.to(dev), table.to(dev), do.to(dev)
    o = K.window_attention_fwd(q, t, *shape)
    dqkv, dtable = K.window_attention_bwd(g, q, t, *shape)
    return o, dqkv, dtable


@pytest.mark.parametrize("name", list(CASES))
def test_window_attention_against_float64(name):
    (B, Hs, Ws, H, _), _, _, _, (ro, rdqkv, rdt) = case(name)
    o, dqkv, dtable = (t.cpu() for t in run(name))
    S = Hs * Ws
    errs = {"O": AC.slice_err(o.reshape(B, S, H, D), ro.reshape(B, S, H, D),
                              AC.FLOOR_FRAC * float(ro.abs().max()))[0]}
    floor = AC.FLOOR_FRAC * float(rdqkv.abs().max())
    a, r = dqkv.reshape(B, S, 3, H, D), rdqkv.reshape(B, S, 3, H, D)
    for i, n in enumerate(("dQ", "dK", "dV")):
        errs[n] = AC.slice_err(a[:, :, i], r[:, :, i], floor)[0]
    errs["dtable"] = float((dtable.double() - rdt).abs().max() / rdt.abs().max())
    print(name, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["O"] < AC.O_TOL
    assert max(errs["dQ"], errs["dK"], errs["dV"]) < AC.DQKV_TOL
    assert errs["dtable"] < DTABLE_TOL


@pytest.mark.parametrize("name", ["all_regions", "past_caps"])
def test_launches_repeat_bit_for_bit(name):
    from mipipe.ops.determinism import deterministic
    first = run(name)
    with deterministic(True):
        det = run(name)
    for a, b, c in zip(first, run(name), det):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_zero_gradient_window_and_accumulating_table():
    shape, qkv, table, do, _ = case("all_regions")
    B, Hs, Ws, H, shift = shape
    idx = _ref.window_geometry(Hs, Ws, shift)[0][3]  # the wrapped corner window of sample 0
    g = do.clone()
    g[idx] = 0
    q, t = qkv.to(dev), table.to(dev)
    dqkv, dtable = K.window_attention_bwd(g.to(dev), q, t, *shape)
    assert not dqkv[idx.to(dev)].any() and dqkv.any()
    acc = torch.full((169 * H,), 2.0, device=dev)
    _, none = K.window_attention_bwd(g.to(dev), q, t, *shape, dtable=acc)
    assert none is None and torch.equal(acc.reshape(169, H), dtable + 2.0)


def test_unshifted_map_equals_its_windows_alone():
    g = torch.Generator().manual_seed(3)
    H, t = 2, torch.randn(169, 2, generator=g).to(dev)
    qkv = torch.randn(14, 14, 3 * H * D, generator=g).to(torch.bfloat16).to(dev)
    o = K.window_attention_fwd(qkv.reshape(196, -1), t, 1, 14, 14, H, 0).reshape(14, 14, -1)
    for y in (0, 7):
        for x in (0, 7):
            part = qkv[y:y + 7, x:x + 7].reshape(49, -1).contiguous()
            alone = K.window_attention_fwd(part, t, 1, 7, 7, H, 0)
            assert torch.equal(o[y:y + 7, x:x + 7].reshape(49, -1), alone)


@pytest.mark.parametrize("hw", [(2, 2), (6, 10), (14, 14)])
@pytest.mark.parametrize("C", [8, 96, 136])
def test_patch_merge_bit_for_bit(C, hw):
    B, (Hs, Ws) = 3, hw
    x = torch.randn(B * Hs * Ws, C).to(torch.bfloat16)
    y = K.patch_merge(x.to(dev), B, Hs, Ws)
    assert torch.equal(y.cpu(), _ref.patch_merge(x, B, Hs, Ws))
    dy = torch.randn(B * Hs * Ws // 4, 4 * C).to(torch.bfloat16)
    dx = K.patch_merge(dy.to(dev), B, Hs, Ws, bwd=True)
    assert torch.equal(dx.cpu(), _ref.patch_merge_bwd(dy, B, Hs, Ws))


@pytest.mark.parametrize("what,match", [
    ("map", "7x7 windows"), ("shift", "0 or 3"), ("cols", "head width 32"),
    ("align", "16-byte"), ("large", "2\\^31"), ("empty", "empty"), ("odd", "even sides")])
def test_argument_checks(what, match):
    C = native()
    t = torch.zeros(169, device=dev)
    z = lambda r, c: torch.zeros(r, c, dtype=torch.bfloat16, device=dev)  # noqa: E731
    with pytest.raises(RuntimeError, match=match):
        if what == "map":
            C.winattn_fwd(z(8 * 7, 96), t, 1, 8, 7, 1, 0, 0)
        elif what == "shift":
            C.winattn_fwd(z(49, 96), t, 1, 7, 7, 1, 2, 0)
        elif what == "cols":
            C.winattn_fwd(z(49, 192), t, 1, 7, 7, 1, 0, 0)
        elif what == "align":
            C.winattn_fwd(z(50, 96).reshape(-1)[4:4 + 49 * 96].reshape(49, 96), t, 1, 7, 7, 1, 0, 0)
        elif what == "large":
            C.winattn_fwd(z(49, 96), t, 2 ** 19, 7, 7, 1, 0, 0)
        elif what == "empty":
            C.winattn_fwd(z(0, 96), t, 0, 7, 7, 1, 0, 0)
        else:
            C.patch_merge(z(15, 8), 1, 3, 5)
