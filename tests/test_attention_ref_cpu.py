"""The float64 attention reference of attention_common.py, checked without a GPU: against torch
autograd, against the trusted fp32 reference (_ref), and the attainability of the GPU sweep's
tolerances by a bf16 model of the kernel design.  Also measures the fp32 lse error that sets the
sweep's lse tolerance."""
import math

import pytest
import torch

import attention_common as AC
from attention_common import D, SCALE
from mipipe.ops import _ref


def _autograd(qkv, do, B, S, H, mask, scale, keep, p_drop):
    x = qkv.double().requires_grad_(True)
    t = x.reshape(B, S, 3, H, D)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) * scale
    if mask is not None:
        s = s + mask.double().reshape(B, 1, 1, S)
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep.double() / (1.0 - p_drop)
    o = (p @ v).transpose(1, 2).reshape(B * S, H * D)
    o.backward(do.double())
    return o.detach(), torch.logsumexp(s, -1).detach(), x.grad


# a one-key sample has nothing to mask
_SM = [(1, "none")] + [(S, mk) for S in (33, 129) for mk in ("none", "ragged", "lead")]


@pytest.mark.parametrize("S,mask_kind", _SM)
@pytest.mark.parametrize("drop", [False, True])
def test_reference_matches_autograd(S, mask_kind, drop):
    B, H = 2, 2
    qkv, do, mask = AC.make_case(B, S, H, mask_kind, 7 + S)
    p_drop = 0.1 if drop else 0.0
    keep = _ref.attention_keep(B, S, H, p_drop, 99, "cpu") if drop else None
    o, lse, dqkv = AC.attention_f64(qkv, do, B, S, H, mask, SCALE, keep, p_drop)
    o_a, lse_a, d_a = _autograd(qkv, do, B, S, H, mask, SCALE, keep, p_drop)
    assert (o - o_a).abs().max().item() < 1e-10
    assert (lse - lse_a).abs().max().item() < 1e-10
    HD = H * D
    for i, name in enumerate(("dq", "dk", "dv")):
        e = (dqkv[:, i * HD:(i + 1) * HD] - d_a[:, i * HD:(i + 1) * HD]).abs().max().item()
        assert e < 1e-10, (name, e)


@pytest.mark.parametrize("mask_kind", ["ragged_inf", "lead_inf"])
def test_reference_inf_mask_no_nan_and_matches_autograd(mask_kind):
    """-inf biases: exact zeros for the masked keys, no NaN while a row keeps a key."""
    B, S, H = 2, 129, 2
    qkv, do, mask = AC.make_case(B, S, H, mask_kind, 5)
    o, lse, dqkv = AC.attention_f64(qkv, do, B, S, H, mask, SCALE)
    assert all(bool(torch.isfinite(t).all()) for t in (o, lse, dqkv))
    o_a, lse_a, d_a = _autograd(qkv, do, B, S, H, mask, SCALE, None, 0.0)
    assert (o - o_a).abs().max().item() < 1e-10
    assert (lse - lse_a).abs().max().item() < 1e-10
    assert (dqkv - d_a).abs().max().item() < 1e-10
    masked = ~AC.kept_keys(B, S, mask_kind)
    kv = dqkv.reshape(B, S, 3, H * D)[:, :, 1:]
    assert torch.count_nonzero(kv[masked]) == 0


def test_reference_empty_sample():
    """Every key of sample 1 at -inf: O = 0, lse = -inf, zero gradient, no NaN; sample 0 as if
    alone."""
    B, S, H = 2, 65, 2
    qkv, do, _ = AC.make_case(B, S, H, "none", 3)
    mask = torch.zeros(B, S)
    mask[1] = -math.inf
    o, lse, dqkv = AC.attention_f64(qkv, do, B, S, H, mask, SCALE)
    assert not torch.isnan(o).any() and not torch.isnan(dqkv).any()
    assert torch.count_nonzero(o[S:]) == 0 and torch.count_nonzero(dqkv[S:]) == 0
    assert bool((lse[1] == -math.inf).all())
    o0, lse0, d0 = AC.attention_f64(qkv[:S], do[:S], 1, S, H, None, SCALE)
    assert torch.equal(o[:S], o0) and torch.equal(lse[0], lse0[0]) and torch.equal(dqkv[:S], d0)


@pytest.mark.parametrize("S,mask_kind", [c for c in _SM if c[1] != "lead"])
@pytest.mark.parametrize("drop", [False, True])
def test_reference_matches_fp32_ref(S, mask_kind, drop):
    """Ties the float64 reference to the fp32 one the suite already trusts (given the float64
    o / lse, as the kernel tests give it the kernel's)."""
    B, H = 2, 3
    qkv, do, mask = AC.make_case(B, S, H, mask_kind, 11 + S)
    p_drop, seed = (0.1, 42) if drop else (0.0, 0)
    keep = _ref.attention_keep(B, S, H, p_drop, seed, "cpu") if drop else None
    o, lse, dqkv = AC.attention_f64(qkv, do, B, S, H, mask, SCALE, keep, p_drop)
    o_r, lse_r = _ref.attention_fwd(qkv.float(), B, S, H, mask, SCALE, p_drop, seed)
    d_r = _ref.attention_bwd(do.float(), qkv.float(), o.float(), lse.float(), B, S, H, mask,
                             SCALE, p_drop, seed)
    for name, a, r in (("o", o_r, o), ("lse", lse_r, lse), ("dqkv", d_r, dqkv)):
        e = ((a.double() - r).abs().max() / r.abs().max().clamp_min(1.0)).item()
        assert e < 1e-4, (name, e)


def _all_cases():
    return AC.sweep_cases() + AC.inf_cases()


def test_bf16_model_meets_half_tolerance():
    """Attainability: for every case of the GPU sweep, the reference math with only the roundings
    a bf16 flash kernel cannot avoid passes slice_err at half the GPU tolerances."""
    worst = {}
    for B, S, H, mk in _all_cases():
        qkv, do, mask, ref = AC.case_and_reference(B, S, H, mk)
        o, lse, dqkv = AC.attention_bf16_model(qkv, do, B, S, H, mask, SCALE)
        AC.assert_close_to_reference(o, None, dqkv, ref, B, S, H, frac=0.5, what=f"model {mk}")
        for n, (e, _) in AC.tensor_errors(o, dqkv, ref[0], ref[2], B, S, H).items():
            if e > worst.get(n, (0.0, None))[0]:
                worst[n] = (e, (B, S, H, mk))
    print("attainability margins (worst slice error of the bf16 model; tolerance O 2e-2, "
          "dQ/dK/dV 3e-2):", {n: (f"{e:.2e}", c) for n, (e, c) in worst.items()})


def test_lse_fp32_error_sets_tolerance():
    """The largest relative lse error of an fp32 evaluation of the reference over every sweep
    input is what attention_common.LSE_FP32_ERR records (LSE_TOL = 16 x that, below 1e-3)."""
    worst, where = 0.0, None
    for B, S, H, mk in _all_cases():
        qkv, _, mask, ref = AC.case_and_reference(B, S, H, mk)
        e = AC.lse_err(AC.lse_fp32(qkv, B, S, H, mask, SCALE), ref[1])
        if e > worst:
            worst, where = e, (B, S, H, mk)
    print(f"fp32 lse error vs float64: {worst:.3e} at {where}; LSE_FP32_ERR = "
          f"{AC.LSE_FP32_ERR:.2e}, LSE_TOL = {AC.LSE_TOL:.2e}")
    assert worst <= AC.LSE_FP32_ERR <= 4 * worst, worst  # the constant is the measurement
    assert AC.LSE_TOL == 16 * AC.LSE_FP32_ERR and AC.LSE_TOL < 1e-3


def test_slice_err_floor_and_nan():
    """An identically-zero slice divides by the floor, not by zero; NaN is the worst error."""
    ref = torch.zeros(2, 4, 2, D, dtype=torch.float64)
    ref[0, :, 0] = 1.0
    a = ref.clone()
    a[1, 0, 1, 0] = 0.05  # a zero slice off by 0.05: 0.05 / floor
    e, where = AC.slice_err(a, ref, 0.25)
    assert where == (1, 1) and abs(e - 0.2) < 1e-12
    a[0, 0, 0, 0] = math.nan
    e, where = AC.slice_err(a, ref, 0.25)
    assert e == math.inf and where == (0, 0)


def test_make_case_masks():
    B, S = 2, 129
    kept = AC.kept_keys(B, S, "ragged")
    assert kept.sum(1).tolist() == [43, 86] and bool(kept[:, 0].all())
    assert AC.kept_keys(3, 2, "ragged").sum(1).tolist() == [1, 1, 1]  # at least one key
    assert AC.kept_keys(B, S, "lead").sum(1).tolist() == [59, 59]
    assert AC.kept_keys(B, 31, "lead").sum(1).tolist() == [1, 1]
    m, mi = AC.make_mask(B, S, "ragged"), AC.make_mask(B, S, "ragged_inf")
    assert bool((m[~kept] == -10000.0).all()) and bool((mi[~kept] == -math.inf).all())
    assert bool((m[kept] == 0).all()) and bool((mi[kept] == 0).all())
