"""The design of the BatchNorm edge tests (bn_common.py, used by test_bn_edges_gpu.py), proved
without a GPU:

* the mirrored launch geometry puts every shape on the edge it is named after;
* the integer constructions are exact: the float64 results are fp32 (and bf16) numbers, the sums
  of magnitudes stay below 2^24 steps, and an fp32 evaluation in the kernels' own operation order
  reproduces them bit for bit;
* a defective reference (a batch-statistic term, the second branch's mean, the residual affine
  dropped; a row lost or counted twice) differs from the true one in EVERY exact case, so a kernel
  with that defect cannot pass;
* on the random cases an fp32 evaluation in the kernels' order of operations stays inside every
  stated bound: the reference alone passes.
"""
import pytest
import torch

import bn_common as bc
from bn_common import CPU_CONSTS as K

BF16 = torch.bfloat16
MODES = (0, 1, 2)


def _fwd_args(d, mode):
    r = None if mode == 0 else d.r
    return (d.y, d.scale, d.bias, r, d.rscale if mode == 2 else None,
            d.rbias if mode == 2 else None)


def _apply_kw(d, mode):
    return dict(y2=d.y2, mean2=d.mean2, invstd2=d.invstd2, gamma2=d.gamma2,
                sum_gx2=d.sum_gx2) if mode == 2 else {}


@pytest.mark.parametrize("C", bc.C_LIST)
def test_shapes_cross_their_edges(C):
    for u in (2, 4):
        bc.apply_rows(C, u, K)
    bc.reduce_rows(C, K)
    tpr, rpb, passes = bc.row_map(C, K)
    assert {8: rpb == 256, 40: tpr * rpb == 255, 1000: tpr * rpb == 250, 2056: passes == 2,
            4096: passes == 2}.get(C, True)


def test_cap_and_det_cases():
    names = [c[0] for c in bc.cap_cases(K)] + [c[0] for c in bc.det_cases(K)]
    assert names == ["budget", "budget_2pass", "floor", "block_cap", "sum16_tails", "chunk_sums"]


@pytest.mark.parametrize("C", bc.C_LIST)
def test_forward_exact_and_sensitive(C):
    for u in (2, 4):
        for M in sorted(set(bc.apply_rows(C, u, K).values())):
            d = bc.exact_inputs(C, M)
            for mode in MODES:
                for relu in (True, False):
                    args = _fwd_args(d, mode)
                    z, T = bc.ref_fwd(*args, relu)
                    bc.assert_exact(z, T * 2, stored=BF16)          # every term a multiple of 1/2
                    assert z.abs().max() <= 17
                    f = [None if t is None else t.float() for t in args]
                    assert torch.equal(bc.model_fwd_fp32(*f, relu, BF16).double(), z)
                    mutants = ["bias"] + (["res"] if mode else []) + (["res_affine"] if mode == 2 else [])
                    for mutant in mutants:
                        assert not torch.equal(bc.ref_fwd(*args, relu, mutant=mutant)[0], z), \
                            (C, M, mode, relu, mutant)
    d = bc.exact_inputs(64, 191)
    pos = (bc.ref_fwd(*_fwd_args(d, 2), True)[0] > 0).double().mean().item()
    assert 0.3 < pos < 0.55, pos       # the mask bits are neither all set nor all clear


@pytest.mark.parametrize("C", bc.C_LIST)
def test_apply_exact_and_sensitive(C):
    for u in (2, 4):
        for M in sorted(set(bc.apply_rows(C, u, K).values())):
            d = bc.exact_inputs(C, M)
            for mode in MODES:
                for relu in (True, False):
                    z = d.z if relu else d.zneg
                    base = (d.dz, z, d.y, d.mean, d.invstd, d.gamma, d.sum_g, d.sum_gx, d.count, relu)
                    o = bc.ref_apply(*base, **_apply_kw(d, mode))
                    # smallest step: a >= 1/4 times an inner step of 1/8 (see ref_apply's form)
                    bc.assert_exact(o.dy, o.T * 32, stored=BF16)
                    assert o.dy.abs().max() <= 42
                    g32 = o.g.float()
                    m = bc.model_apply_fp32(g32, d.y.float(), d.mean.float(), d.invstd.float(),
                                            d.gamma.float(), d.sum_g.float(), d.sum_gx.float(),
                                            d.count, BF16)
                    assert torch.equal(m.double(), o.dy)
                    mutants = ["k1", "k2", "mean"]
                    if mode == 2:
                        bc.assert_exact(o.dy2, o.T2 * 32, stored=BF16)
                        m = bc.model_apply_fp32(g32, d.y2.float(), d.mean2.float(),
                                                d.invstd2.float(), d.gamma2.float(),
                                                d.sum_g.float(), d.sum_gx2.float(), d.count, BF16)
                        assert torch.equal(m.double(), o.dy2)
                        mutants += ["mean2", "k22"]
                    for mutant in mutants:
                        w = bc.ref_apply(*base, **_apply_kw(d, mode), mutant=mutant)
                        same = torch.equal(w.dy, o.dy) and (mode != 2 or torch.equal(w.dy2, o.dy2))
                        assert not same, (C, M, mode, relu, mutant)
                    if mode == 2:   # k1 reaches both branches
                        w = bc.ref_apply(*base, **_apply_kw(d, mode), mutant="k1")
                        assert not torch.equal(w.dy2, o.dy2)


def _reduce_cases():
    cases = [(C, M, False) for C in bc.C_LIST for M in sorted(set(bc.reduce_rows(C, K).values()))]
    cases += [(C, M, small) for _, C, M, small in bc.cap_cases(K)]
    cases += [(C, M, False) for _, C, M in bc.det_cases(K)]
    return cases


def test_reduce_exact_and_sensitive():
    for C, M, small in _reduce_cases():
        if M * C > 1 << 24:
            # the block-cap case: too large to build here; its exactness is a matter of ranges
            assert small
            d = bc.exact_inputs(C, 64, small=True)
            assert M * d.term_max / d.term_step < bc.EXACT
            continue
        d = bc.exact_inputs(C, M, small)
        assert bc.reduce_exact_bound(d) < bc.EXACT, (C, M)
        for relu in (True, False):
            z = d.z if relu else d.zneg
            args = (d.dz, z, d.y, d.mean, d.invstd, relu, d.y2, d.mean2, d.invstd2)
            o = bc.ref_reduce(*args)
            for s, a in ((o.sg, o.ag), (o.sgx, o.agx), (o.sgx2, o.agx2)):
                bc.assert_exact(s, a / d.term_step)
                assert a.max() / d.term_step <= bc.reduce_exact_bound(d)
            for mutant in ("drop_row", "dup_row"):
                w = bc.ref_reduce(*args, mutant=mutant)
                assert not torch.equal(w.sg, o.sg), (C, M, relu, mutant)
                assert not torch.equal(w.sgx, o.sgx) and not torch.equal(w.sgx2, o.sgx2)
            if not relu and M * C >= 64:    # a kernel that applied the mask anyway would differ
                assert not torch.equal(bc.ref_reduce(d.dz, z, d.y, d.mean, d.invstd, True).sg, o.sg)


def test_reduce_model_is_exact_on_integer_data():
    """The fp32 model of the reduction's order of additions gives the float64 sums bit for bit on
    an exact case, atomic and deterministic: the model adds every row once."""
    for C, M in ((40, 357), (64, 5000), (2056, 7)):
        d = bc.exact_inputs(C, M)
        o = bc.ref_reduce(d.dz, d.z, d.y, d.mean, d.invstd, True)
        t = (bc.masked_g(d.dz, d.z, True) * (d.y - d.mean) * d.invstd).float()
        for det in (False, True):
            assert torch.equal(bc.model_reduce_fp32(t, C, K, det).double(), o.sgx)


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=lambda t: bc.DT_ID[t])
@pytest.mark.parametrize("case", bc.RANDOM_CASES, ids=lambda c: c[0])
def test_reference_in_fp32_is_inside_the_bounds(case, dtype):
    name, C, M, offset = case
    d = bc.random_inputs(name, C, M, offset, dtype)
    if offset:
        assert (d.mean.abs() * d.invstd).min() > 300      # the B*y + Cc split cancels
    for mode in MODES:
        for relu in (True, False):
            args = _fwd_args(d, mode) if mode < 2 else (d.y, d.scale, d.bias, d.y2, d.rscale, d.rbias)
            z, T = bc.ref_fwd(*args, relu)
            q = bc.worst(bc.model_fwd_fp32(*args, relu, dtype), z, bc.elementwise_bound(z, T, dtype))
            assert q <= 1, ("fwd", mode, relu, q)
            base = (d.dz, d.z, d.y, d.mean, d.invstd, d.gamma, d.sum_g, d.sum_gx, d.count, relu)
            o = bc.ref_apply(*base, **_apply_kw(d, mode))
            g = o.g.to(dtype)
            m = bc.model_apply_fp32(g, d.y, d.mean, d.invstd, d.gamma, d.sum_g, d.sum_gx, d.count, dtype)
            q = bc.worst(m, o.dy, bc.elementwise_bound(o.dy, o.T, dtype))
            assert q <= 1, ("apply", mode, relu, q)
            if mode == 2:
                m = bc.model_apply_fp32(g, d.y2, d.mean2, d.invstd2, d.gamma2, d.sum_g, d.sum_gx2,
                                        d.count, dtype)
                q = bc.worst(m, o.dy2, bc.elementwise_bound(o.dy2, o.T2, dtype))
                assert q <= 1, ("apply2", relu, q)
    o = bc.ref_reduce(d.dz, d.z, d.y, d.mean, d.invstd, True, d.y2, d.mean2, d.invstd2)
    g = bc.masked_g(d.dz, d.z, True).float()
    terms = {"sg": (g, o.sg, o.ag),
             "sgx": (g * (d.y.float() - d.mean) * d.invstd, o.sgx, o.agx),
             "sgx2": (g * (d.y2.float() - d.mean2) * d.invstd2, o.sgx2, o.agx2)}
    for det in (False, True):
        chain = bc.reduce_chain(M, C, K, det)
        for key, (t, ref, mags) in terms.items():
            q = bc.worst(bc.model_reduce_fp32(t, C, K, det), ref, bc.reduce_bound(mags, chain))
            assert q <= 1, (key, det, q)


@pytest.mark.parametrize("count", [1, 4096])
@pytest.mark.parametrize("C", [8, 200, 2056])
def test_finalize_reference_and_tolerance(C, count):
    d = bc.finalize_inputs(C, count, K.replicas)
    o = bc.ref_finalize(d.psum, d.psq, count, d.shift, d.gamma, d.beta, bc.EPS)
    n = bc.NEG_VAR_CHANNEL
    assert o.raw_var[n].item() == -2.0 ** -10 and o.var[n].item() == 0.0
    assert (o.raw_var[torch.arange(C) != n] > 0.3).all()
    mean, var, invstd = bc.model_finalize_fp32(d, bc.EPS)
    assert var[n].item() == 0.0
    assert torch.allclose(mean.double(), o.mean, rtol=1e-5, atol=1e-5)
    assert bc.worst(invstd, o.invstd, o.invstd_tol) <= 1
    # the tolerance is fp32-sized (the existing tests allow 1e-4 .. 1e-5 of the largest value),
    # and for the clamped channel it is the 8 half-ulps alone
    assert (o.invstd_tol / o.invstd).max() < 5e-5
    assert o.invstd_tol[n] == o.invstd[n] * 8 * bc.U24
