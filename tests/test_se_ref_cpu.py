"""The squeeze-excitation / Hardswish contracts of ops/_ref.py (CPU): float64 parity with torch
autograd of the plain composition, torch's one-sided rules at the knees, and the exactness of the
integer constructions the GPU tests rely on."""
import pytest
import torch
import torch.nn.functional as F

from mipipe.ops import _ref

import se_common as S

RTOL = 1e-12


def _close(a, b, what):
    scale = max(1.0, b.abs().max().item())
    assert (a - b).abs().max().item() <= RTOL * scale, what


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _compose(y, gamma, beta, wg, act, training, rm=None, rv=None, eps=1e-3, gate_leaf=None):
    """Plain torch on NCHW: batch_norm -> act -> mean -> gate -> hardsigmoid multiply."""
    N, H, W, C = y.shape
    if training:
        b = F.batch_norm(_nchw(y), None, None, gamma, beta, True, 0.0, eps)
    else:
        b = F.batch_norm(_nchw(y), rm, rv, gamma, beta, False, 0.0, eps)
    z = F.hardswish(b) if act == "hardswish" else F.relu(b)
    pm = z.mean(dim=(2, 3))
    gate = pm @ wg if gate_leaf is None else gate_leaf
    return z * F.hardsigmoid(gate).reshape(N, C, 1, 1), gate


def _ref_chain(y, gamma, beta, wg, act, w_out, mean, invstd, batch_stats, gate_leaf=None,
               drop_dpm=False, drop_xhat=False):
    """The same through the _ref contracts -> (out, dy, dgamma, dbeta, dwg | dgate)."""
    scale = gamma * invstd
    bias = beta - mean * scale
    z, pm = _ref.bn_act_pool_fwd(y, scale, bias, act, True)
    gate = pm @ wg if gate_leaf is None else gate_leaf
    out = _ref.se_scale_fwd(z, gate)
    dz, dgate = _ref.se_scale_bwd(w_out, z, gate)
    dpm = None if (gate_leaf is not None or drop_dpm) else dgate @ wg.t()
    sg, sgx = _ref.bn_act_pool_bwd_reduce(dz, y, scale, bias, mean, invstd, act, dpm)
    sums = (sg, torch.zeros_like(sgx) if drop_xhat else sgx) if batch_stats else (None, None)
    dy = _ref.bn_act_pool_bwd_apply(dz, y, scale, bias, mean, invstd, gamma, act, dpm, *sums)
    dwg = pm.t() @ dgate if gate_leaf is None else dgate
    return out, dy, sgx, sg, dwg


@pytest.mark.parametrize("act", ["relu", "hardswish"])
def test_float64_parity_with_autograd_training_stats(act):
    torch.manual_seed(0)
    N, H, W, C, eps = 3, 5, 7, 16, 1e-3
    y = (torch.randn(N, H, W, C, dtype=torch.float64) * 3).requires_grad_()
    gamma = (torch.rand(C, dtype=torch.float64) + 0.5).requires_grad_()
    beta = torch.randn(C, dtype=torch.float64).requires_grad_()
    wg = torch.randn(C, C, dtype=torch.float64).requires_grad_()
    w_out = torch.randn(N, H, W, C, dtype=torch.float64)
    out, _ = _compose(y, gamma, beta, wg, act, True, eps=eps)
    (out * _nchw(w_out)).sum().backward()
    yd = y.detach()
    mean = yd.reshape(-1, C).mean(0)
    invstd = torch.rsqrt(yd.reshape(-1, C).var(0, unbiased=False) + eps)
    got = _ref_chain(yd, gamma.detach(), beta.detach(), wg.detach(), act, w_out, mean, invstd, True)
    _close(_nchw(got[0]), out.detach(), "out")
    _close(got[1], y.grad, "dy")
    _close(got[2], gamma.grad, "dgamma")
    _close(got[3], beta.grad, "dbeta")
    _close(got[4], wg.grad, "dgate through the FC")
    # the test bites: without the pooled-gradient addend, or without the xhat term, dy is wrong
    scale = y.grad.abs().max().item()
    for kw in (dict(drop_dpm=True), dict(drop_xhat=True)):
        bad = _ref_chain(yd, gamma.detach(), beta.detach(), wg.detach(), act, w_out, mean, invstd,
                         True, **kw)
        assert (bad[1] - y.grad).abs().max().item() > 1e-6 * scale, kw


@pytest.mark.parametrize("act", ["relu", "hardswish"])
def test_float64_knees_with_running_stats(act):
    """u exactly at -3, 0, 3 and gate exactly at -3 and 3: torch's one-sided rules decide."""
    torch.manual_seed(1)
    N, H, W, C = 2, 3, 4, 8
    knees = torch.tensor([-3.0, 0.0, 3.0, -5.0, 4.0, 6.0, 1.25, -1.5], dtype=torch.float64)
    y = knees[torch.randint(0, 8, (N, H, W, C))].requires_grad_()
    gamma = torch.ones(C, dtype=torch.float64).requires_grad_()
    beta = torch.zeros(C, dtype=torch.float64).requires_grad_()
    # var + eps = 1 exactly, so the pre-activation is y itself
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.full((C,), 0.75, dtype=torch.float64)
    gk = torch.tensor([-3.0, 3.0, -4.0, 4.0, 0.5, -2.5], dtype=torch.float64)
    gate = gk[torch.randint(0, 6, (N, C))].requires_grad_()
    w_out = torch.randn(N, H, W, C, dtype=torch.float64)
    out, _ = _compose(y, gamma, beta, None, act, False, rm, rv, eps=0.25, gate_leaf=gate)
    (out * _nchw(w_out)).sum().backward()
    got = _ref_chain(y.detach(), gamma.detach(), beta.detach(), None, act, w_out, rm,
                     torch.ones_like(rv), False, gate_leaf=gate.detach())
    _close(_nchw(got[0]), out.detach(), "out")
    _close(got[1], y.grad, "dy")
    _close(got[2], gamma.grad, "dgamma")
    _close(got[3], beta.grad, "dbeta")
    _close(got[4], gate.grad, "dgate")
    assert (y.detach() == -3).any() and (y.detach() == 3).any() and (y.detach() == 0).any()
    assert (gate.detach() == -3).any() and (gate.detach() == 3).any()


def test_pool_false_returns_no_pm():
    y = torch.randn(1, 2, 2, 8)
    z, pm = _ref.bn_act_pool_fwd(y, torch.ones(8), torch.zeros(8), "hardswish", False)
    assert pm is None and torch.equal(z, F.hardswish(y))
    with pytest.raises(ValueError):
        _ref.bn_act_pool_fwd(y, torch.ones(8), torch.zeros(8), "relu6")


@pytest.mark.parametrize("shape", S.exact_shapes())
@pytest.mark.parametrize("act", ["relu", "hardswish"])
def test_exact_integer_constructions_are_exact(shape, act):
    """The premise of the GPU exact-sum tests: every term a multiple of a quantum, the absolute
    terms below 2^24 quanta — and fp32 _ref, summing in torch's order and in a shuffled order,
    lands on the float64 sums."""
    N, H, W, C = shape
    on = S.is_pow2(H * W)
    c = S.exact_bn_case(N, H, W, C, seed=3, with_dpm=on)
    z, g, gx = S.exact_bn_terms(c, act)
    S.assert_exact_terms(z, 1.0, (1, 2))
    S.assert_exact_terms(g, 0.5, (0, 1, 2))
    S.assert_exact_terms(gx, 0.25, (0, 1, 2))
    f = {k: (None if v is None else v.float()) for k, v in c.items()}
    scale, bias = f["scale"], f["bias"]
    perm = torch.randperm(H * W)
    for order in (slice(None), perm):
        yy = f["y"].reshape(N, H * W, C)[:, order].reshape(N, H, W, C)
        dd = f["dz"].reshape(N, H * W, C)[:, order].reshape(N, H, W, C)
        zf, pm = _ref.bn_act_pool_fwd(yy, scale, bias, act, True)
        want_pm = (z.sum((1, 2)) * float(torch.tensor(1.0 / (H * W), dtype=torch.float32))).float()
        assert torch.equal(pm, want_pm)
        sg, sgx = _ref.bn_act_pool_bwd_reduce(dd, yy, scale, bias, f["mean"], f["invstd"], act,
                                              f["dpm"])
        assert torch.equal(sg.double(), g.sum((0, 1, 2)))
        assert torch.equal(sgx.double(), gx.sum((0, 1, 2)))
    assert torch.equal(zf.double().reshape(N, H * W, C),
                       z.reshape(N, H * W, C)[:, perm])
    zz, dout, gate = S.exact_scale_case(N, H, W, C, seed=4)
    S.assert_exact_terms(dout * zz, 1.0, (1, 2))
    _, dgate = _ref.se_scale_bwd(dout.float(), zz.float(), gate.float())
    sp = ((gate > -3) & (gate < 3)).double() * float(torch.tensor(1.0 / 6, dtype=torch.float32))
    assert torch.equal(dgate, ((dout * zz).sum((1, 2)) * sp).float())
