"""Swin V2's cosine window attention (csrc/kernels/winattn8.hip) on the GPU: forward + backward
against the float64 reference of the bf16-rounded inputs (attention_common's per-slice measure and
tolerances), its exact properties, and the host argument checks."""
import functools
import math

import pytest
import torch

import attention_common as AC
from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu
dev = "cuda"
D = 32
LOGIT_SCALES = (math.log(10.0), math.log(200.0), -1.0)  # the second is clamped at ln 100


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"


def _past_caps():
    """The partial last group (idle waves) and the grid stride; one 8x8 window per sample."""
    C = native()
    return (C.WIN8_RUN * C.WIN8_MAX_RUNS + C.WIN8_RUN + 1, 8, 8, 1, (0, 0))


CASES = {"one_window": (1, 8, 8, 1, (0, 0)), "all_regions": (2, 16, 16, 3, (4, 4)),
         "non_square": (1, 16, 24, 2, (4, 4)), "single_window_axis": (1, 8, 16, 2, (0, 4)),
         "past_caps": _past_caps}


@functools.lru_cache(maxsize=None)
def case(name):
    """(shape, qkv, bias, logit_scale, do on the CPU, float64 (o, dqkv, dbias, dls)); read-only."""
    shape = CASES[name]() if callable(CASES[name]) else CASES[name]
    B, Hs, Ws, H, shift = shape
    g = torch.Generator().manual_seed(Hs * 100 + Ws * 10 + H)
    T = B * Hs * Ws
    qkv = (torch.randn(T, 3 * H * D, generator=g) * 1.5).to(torch.bfloat16)
    do = torch.randn(T, H * D, generator=g).to(torch.bfloat16)
    bias = 16 * torch.sigmoid(torch.randn(225, H, generator=g))
    ls = torch.tensor([LOGIT_SCALES[i % 3] for i in range(H)])
    ref = _ref.window_attention_v2(qkv.double(), bias.double(), ls.double(), B, Hs, Ws, H, shift,
                                   do.double())
    return shape, qkv, bias, ls, do, ref


def run(name):
    shape, qkv, bias, ls, do, _ = case(name)
    q, b, s, g = qkv.to(dev), bias.to(dev), ls.to(dev), do.to(dev)
    o = K.window_attention_v2_fwd(q, b, s, *shape)
    return (o,) + tuple(K.window_attention_v2_bwd(g, q, b, s, *shape))


@pytest.mark.parametrize("name", list(CASES))
def test_window_attention_v2_against_float64(name):
    """V1's bounds, unloosened.  Measured on an MI355X, the worst of the five cases: O 6.1e-3,
    dQ / dK / dV 6.5e-3 (past_caps), dbias 1.2e-6, dlogit_scale 5.0e-6 (single_window_axis)."""
    (B, Hs, Ws, H, _), _, _, _, _, (ro, rdqkv, rdb, rdl) = case(name)
    o, dqkv, dbias, dls = (t.cpu() for t in run(name))
    S = Hs * Ws
    errs = {"O": AC.slice_err(o.reshape(B, S, H, D), ro.reshape(B, S, H, D),
                              AC.FLOOR_FRAC * float(ro.abs().max()))[0]}
    floor = AC.FLOOR_FRAC * float(rdqkv.abs().max())
    a, r = dqkv.reshape(B, S, 3, H, D), rdqkv.reshape(B, S, 3, H, D)
    for i, n in enumerate(("dQ", "dK", "dV")):
        errs[n] = AC.slice_err(a[:, :, i], r[:, :, i], floor)[0]
    errs["dbias"] = float((dbias.double() - rdb).abs().max() / rdb.abs().max())
    errs["dlogit_scale"] = float((dls.double() - rdl).abs().max() / rdl.abs().max())
    print(name, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert errs["O"] < AC.O_TOL
    assert max(errs["dQ"], errs["dK"], errs["dV"]) < AC.DQKV_TOL
    # fp32 sums of fp32 dS, relative to the largest |reference|: the attention gradients' bound
    assert max(errs["dbias"], errs["dlogit_scale"]) < AC.DQKV_TOL


@pytest.mark.parametrize("name", ["all_regions", "past_caps"])
def test_launches_repeat_bit_for_bit(name):
    from mipipe.ops.determinism import deterministic
    first = run(name)
    with deterministic(True):
        det = run(name)
    for a, b, c in zip(first, run(name), det):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_clamped_head_and_accumulating_gradients():
    shape, qkv, bias, ls, do, _ = case("all_regions")
    H = shape[3]
    q, b, s, g = qkv.to(dev), bias.to(dev), ls.to(dev), do.to(dev)
    _, dbias, dls = K.window_attention_v2_bwd(g, q, b, s, *shape)
    assert float(dls[1]) == 0.0 and dls[0] != 0 and dls[2] != 0  # head 1: ln 200 > ln 100
    accb, accl = torch.full((225, H), 2.0, device=dev), torch.full((H,), -3.0, device=dev)
    _, nb, nl = K.window_attention_v2_bwd(g, q, b, s, *shape, dbias=accb, dlogit_scale=accl)
    assert nb is None and nl is None
    assert torch.equal(accb, dbias + 2.0) and torch.equal(accl, dls - 3.0)


def test_unshifted_map_equals_its_windows_alone():
    g, H = torch.Generator().manual_seed(3), 2
    b, s = (16 * torch.rand(225, H, generator=g)).to(dev), torch.tensor([2.0, -1.0], device=dev)
    qkv = torch.randn(16, 16, 3 * H * D, generator=g).to(torch.bfloat16).to(dev)
    o = K.window_attention_v2_fwd(qkv.reshape(256, -1), b, s, 1, 16, 16, H, 0).reshape(16, 16, -1)
    for y in (0, 8):
        for x in (0, 8):
            part = qkv[y:y + 8, x:x + 8].reshape(64, -1).contiguous()
            alone = K.window_attention_v2_fwd(part, b, s, 1, 8, 8, H, 0)
            assert torch.equal(o[y:y + 8, x:x + 8].reshape(64, -1), alone)


def test_zero_query_row_is_softmax_of_bias_and_mask():
    shape, qkv, bias, ls, _, _ = case("all_regions")
    H = shape[3]
    z = qkv.clone()
    z[5, :H * D] = 0   # every head's q of one token
    z[200, :D] = 0     # head 0's q of a token of a wrapped window
    o = K.window_attention_v2_fwd(z.to(dev), bias.to(dev), ls.to(dev), *shape).cpu()
    ro = _ref.window_attention_v2(z.double(), bias.double(), ls.double(), *shape)
    assert bool(torch.isfinite(o).all())
    for row in (5, 200):
        assert float((o[row].double() - ro[row]).abs().max()) < AC.O_TOL * float(ro.abs().max())


@pytest.mark.parametrize("match,rows,hs,ws,sy,bias_rows,ls_n", [
    ("8x8 windows", 96, 8, 12, 0, 225, 1), ("0 or 4", 64, 8, 8, 3, 225, 1),
    (r"bias must be \[225, 1\]", 64, 8, 8, 0, 169, 1),
    (r"logit_scale must be \[1\]", 64, 8, 8, 0, 225, 2), ("empty", 0, 8, 8, 0, 225, 1)])
def test_argument_checks(match, rows, hs, ws, sy, bias_rows, ls_n):
    qkv = torch.zeros(rows, 96, dtype=torch.bfloat16, device=dev)
    b, s = torch.zeros(bias_rows, 1, device=dev), torch.zeros(ls_n, device=dev)
    with pytest.raises(RuntimeError, match=match):
        native().winattn8_fwd(qkv, b, s, 1 if rows else 0, hs, ws, 1, sy, 0)
