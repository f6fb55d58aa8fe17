"""attention.hip against an independent float64 reference (tests/attention_common.py) over the
sequence lengths where its kernels change path, per-sample / leading / -inf masks, 12 heads,
deterministic dQ slabs; exact properties of masks, padding and the dropout hash indexing.

Regimes by S: forward query block 32*NW (64 / 128), forward K/V tile 64, backward key block
32*NW, backward query tile 32, direct dQ (S <= 64 with 2 waves, <= 128 with 4), S = 2048 (the
forward's LDS mask image exactly full).  The backward always gets the kernel's own o / lse, as
in training; the reference gradients never see them."""
import math

import pytest
import torch

import attention_common as AC
from attention_common import D, SCALE
from mipipe.ops import _ref
from mipipe.ops._native import native, native_available
from mipipe.ops.determinism import deterministic

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"


@pytest.fixture(params=[2, 4], ids=["2waves", "4waves"])
def attn_waves(request):
    """Both attention block shapes (32 rows per wave)."""
    native().set_attn_waves(request.param)
    yield request.param
    native().set_attn_waves(0)


def _fwd(qkv, mask, B, S, H, p=0.0, seed=0):
    m = None if mask is None else mask.to(dev)
    return native().attention_fwd(qkv.to(dev), B, S, H, m, SCALE, p, seed)


def _fwd_bwd(qkv, do, mask, B, S, H, p=0.0, seed=0):
    """(o, lse, dqkv) on the CPU; the backward reads the kernel's own o / lse."""
    m = None if mask is None else mask.to(dev)
    q = qkv.to(dev)
    o, lse = native().attention_fwd(q, B, S, H, m, SCALE, p, seed)
    dqkv = native().attention_bwd(do.to(dev), q, o, lse, B, S, H, m, SCALE, p, seed)
    return o.cpu(), lse.cpu(), dqkv.cpu()


def _id(c):
    return f"B{c[0]}-S{c[1]}-H{c[2]}-{c[3]}"


@pytest.mark.parametrize("case", AC.sweep_cases(), ids=_id)
def test_sweep_vs_float64(case, attn_waves):
    B, S, H, mk = case
    qkv, do, mask, ref = AC.case_and_reference(B, S, H, mk)
    o, lse, dqkv = _fwd_bwd(qkv, do, mask, B, S, H)
    AC.assert_close_to_reference(o, lse, dqkv, ref, B, S, H, what=f"{attn_waves}w {mk}")


@pytest.mark.parametrize("case", AC.inf_cases(), ids=_id)
def test_masked_keys_get_exactly_zero_gradient(case, attn_waves):
    """exp2 of a bias <= -14427 underflows to 0 in fp32 for scores of order 10, and -inf gives 0
    by definition: dK and dV of a masked key are exactly 0.0, and the rest meets the tolerances."""
    B, S, H, mk = case
    qkv, do, mask, ref = AC.case_and_reference(B, S, H, mk)
    o, lse, dqkv = _fwd_bwd(qkv, do, mask, B, S, H)
    masked = ~AC.kept_keys(B, S, mk)
    assert masked.any()
    dkv = dqkv.reshape(B, S, 3, H * D)[:, :, 1:]
    assert torch.count_nonzero(dkv[masked]) == 0
    AC.assert_close_to_reference(o, lse, dqkv, ref, B, S, H, what=f"{attn_waves}w {mk}")


@pytest.mark.parametrize("S,L", [(129, 100), (257, 65)])
@pytest.mark.parametrize("neg", [AC.NEG, -math.inf], ids=["m10000", "minf"])
def test_padding_does_not_change_kept_rows(S, L, neg, attn_waves):
    """Rows [0, L) of O and lse of a sample run at S with keys >= L masked are bit-identical to
    the same sample run at S = L: a fully masked tile gives alpha = 1 and a zero row sum, masked
    keys inside a tile add exact zeros."""
    B, H = 2, 2
    qkv, _, _ = AC.make_case(B, S, H, "none", 77)
    mask = torch.zeros(B, S)
    mask[:, L:] = neg
    o, lse = _fwd(qkv, mask, B, S, H)
    short = qkv.reshape(B, S, -1)[:, :L].reshape(B * L, -1).contiguous()
    o_s, lse_s = _fwd(short, None, B, L, H)
    assert torch.equal(o.reshape(B, S, -1)[:, :L], o_s.reshape(B, L, -1))
    assert torch.equal(lse[:, :, :L], lse_s)


def _drop_inputs(B, S, H, seed):
    """q, k small enough that every probability is far from bf16 underflow: a zero in the
    output is a dropped or masked element, nothing else."""
    g = torch.Generator().manual_seed(seed)
    qk = (torch.randn(B * S, 2 * H * D, generator=g) * 0.5).to(torch.bfloat16)
    v = torch.randn(B * S, H * D, generator=g).to(torch.bfloat16)
    return qk, v


DROP_SHAPES = [33, 100, 129, 200]
P_DROP, DROP_SEED = 0.1, 4242


@pytest.mark.parametrize("S", DROP_SHAPES)
@pytest.mark.parametrize("mask_kind", ["none", "ragged"])
def test_dropout_keep_pattern_forward(S, mask_kind, attn_waves):
    """V = one-hot window (key w + j -> e_j): O[q, j] = P[q, w+j] * keep / (1 - p), so the zero
    pattern of O is the keep mask of keys [w, w + 64), for every window covering [0, S)."""
    B, H = 2, 2
    qk, _ = _drop_inputs(B, S, H, S)
    mask = AC.make_mask(B, S, mask_kind)
    kept = AC.kept_keys(B, S, mask_kind)
    keep = _ref.attention_keep(B, S, H, P_DROP, DROP_SEED, "cpu")  # [B, H, q, k]
    for w in range(0, S, D):
        n = min(D, S - w)
        v = torch.zeros(B, S, H, D)
        for j in range(n):
            v[:, w + j, :, j] = 1.0
        qkv = torch.cat([qk, v.reshape(B * S, H * D).to(torch.bfloat16)], 1)
        o, _ = _fwd(qkv, mask, B, S, H, P_DROP, DROP_SEED)
        got = (o.cpu().reshape(B, S, H, D) != 0).permute(0, 2, 1, 3)  # [B, H, q, j]
        want = torch.zeros(B, H, S, D, dtype=torch.bool)
        want[..., :n] = keep[:, :, :, w:w + n] & kept[:, None, None, w:w + n]
        assert torch.equal(got, want), (w, int((got != want).sum()))


@pytest.mark.parametrize("S", DROP_SHAPES)
@pytest.mark.parametrize("mask_kind", ["none", "ragged"])
def test_dropout_keep_pattern_backward(S, mask_kind, attn_waves):
    """dO = one-hot window over queries (query w + j -> e_j): dV[k, j] = P[w+j, k] * keep[w+j, k]
    / (1 - p), so the zero pattern of dV is the transposed keep window: pins the backward's
    row_id (clamped query, S) and key index."""
    B, H = 2, 2
    qk, v = _drop_inputs(B, S, H, 1000 + S)
    qkv = torch.cat([qk, v], 1).to(dev)
    mask = AC.make_mask(B, S, mask_kind)
    m = None if mask is None else mask.to(dev)
    kept = AC.kept_keys(B, S, mask_kind)
    keep = _ref.attention_keep(B, S, H, P_DROP, DROP_SEED, "cpu")
    o, lse = native().attention_fwd(qkv, B, S, H, m, SCALE, P_DROP, DROP_SEED)
    for w in range(0, S, D):
        n = min(D, S - w)
        do = torch.zeros(B, S, H, D)
        for j in range(n):
            do[:, w + j, :, j] = 1.0
        do = do.reshape(B * S, H * D).to(torch.bfloat16).to(dev)
        dqkv = native().attention_bwd(do, qkv, o, lse, B, S, H, m, SCALE, P_DROP, DROP_SEED)
        dv = dqkv.cpu().reshape(B, S, 3, H, D)[:, :, 2]
        got = (dv != 0).permute(0, 2, 1, 3)  # [B, H, k, j]
        want = torch.zeros(B, H, S, D, dtype=torch.bool)
        want[..., :n] = keep[:, :, w:w + n, :].transpose(-1, -2) & kept[:, None, :, None]
        assert torch.equal(got, want), (w, int((got != want).sum()))


@pytest.mark.parametrize("case", [(2, 129, 3), (2, 257, 3), (1, 2048, 2)],
                         ids=lambda c: f"B{c[0]}-S{c[1]}-H{c[2]}")
@pytest.mark.parametrize("mask_kind", ["none", "ragged"])
def test_deterministic_mode_vs_float64(case, mask_kind, attn_waves):
    """Per-key-block dQ slabs + attn_dq_store_kernel (S = 129: a nearly empty last slab) against
    the float64 reference, and two calls bit-identical."""
    B, S, H = case
    qkv, do, mask, ref = AC.case_and_reference(B, S, H, mask_kind)
    with deterministic(True):  # restores the previous mode in its finally
        assert native().get_deterministic()
        o, lse, dqkv = _fwd_bwd(qkv, do, mask, B, S, H)
        _, _, again = _fwd_bwd(qkv, do, mask, B, S, H)
    assert torch.equal(dqkv, again)
    AC.assert_close_to_reference(o, lse, dqkv, ref, B, S, H, what=f"det {attn_waves}w {mask_kind}")


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_empty_sample(det, attn_waves):
    """A sample whose every key is masked with -inf (an all-padding row of a batch): O = 0 and
    lse = -inf by design; its gradient is exactly zero and nothing turns NaN; the other sample's
    results are those of that sample alone."""
    B, S, H = 2, 65, 2
    qkv, do, _ = AC.make_case(B, S, H, "none", 31)
    mask = torch.zeros(B, S)
    mask[1] = -math.inf
    with deterministic(det):
        o, lse, dqkv = _fwd_bwd(qkv, do, mask, B, S, H)
    assert torch.count_nonzero(o[S:]) == 0
    assert bool((lse[1] == -math.inf).all())
    assert bool(torch.isfinite(dqkv.float()).all()), "NaN / Inf in dQKV"
    assert torch.count_nonzero(dqkv[S:]) == 0
    ref0 = AC.attention_f64(qkv[:S], do[:S], 1, S, H, None, SCALE)
    AC.assert_close_to_reference(o[:S], lse[:1], dqkv[:S], ref0, 1, S, H,
                                 what=f"sample 0 {attn_waves}w")
