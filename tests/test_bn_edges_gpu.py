"""bn.hip's training passes (bn_finalize, bn_act_fwd, bn_act_bwd_reduce, bn_act_bwd_apply) at
every launch edge, against float64.

Shapes come from the launch constants the extension exports (``BN_THREADS`` ... ``BN_ROW_ITERS``,
``DET_CHUNK_ROWS``, ``bn_apply_u()``, ``bn_bwd_reduce_blocks()``) through the mirror of the launch
formulas in bn_common.py, and every shape carries the assertion of the edge it crosses: idle
threads (C = 40, 1000), rpb = 256 (C = 8), several channel passes (C > 2048), row tails of the apply
tiles and of the reduction's 4-row trips, the three limits of the reduction's grid, and both paths
of the deterministic collect.

Integer-valued cases are compared with ``torch.equal``: bn_common.py explains why a zero tolerance
is right and test_bn_edges_cpu.py proves it, together with the fact that a reference lacking a
batch-statistic term, the second branch's mean, the residual affine or a row fails every such
case.  Random cases use per-element and per-channel bounds derived there, never a global maximum.

Run on an MI355X:  python -m pytest tests/test_bn_edges_gpu.py -m gpu
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import bn_common as bc
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu
dev = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
dt_id = lambda t: bc.DT_ID[t]
CHILD = "MIPIPE_BN_EDGES_U4_CHILD"     # set in the child of test_u4_instantiations
SENTINEL = 0xA5


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"


def consts():
    n = native()
    return SimpleNamespace(threads=n.BN_THREADS, row_u=n.BN_ROW_U, apply_u=n.BN_APPLY_U,
                           reduce_blocks=n.BN_REDUCE_BLOCKS, atomic_budget=n.BN_ATOMIC_BUDGET,
                           min_blocks=n.BN_MIN_BLOCKS, row_iters=n.BN_ROW_ITERS,
                           det_chunk_rows=n.DET_CHUNK_ROWS, replicas=n.STAT_REPLICAS)


def apply_u():
    return native().bn_apply_u()


def act(t, dtype):
    return None if t is None else t.to(dtype).to(dev)


def vec(t):
    return None if t is None else t.float().to(dev)


def same(out, ref):
    return torch.equal(out.double().cpu(), ref.cpu())


class nt_store:
    """set_nt_store(bits) for the block, the previous value restored."""
    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        self.old = native().get_nt_store()
        native().set_nt_store(self.bits)

    def __exit__(self, *exc):
        native().set_nt_store(self.old)


class deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = native().get_deterministic()
        native().set_deterministic(self.on)

    def __exit__(self, *exc):
        native().set_deterministic(self.old)


def test_apply_u_in_effect():
    want = 4 if os.environ.get("MIPIPE_BN_U", "").strip() == "4" else native().BN_APPLY_U
    assert apply_u() == want
    if os.environ.get(CHILD):
        assert apply_u() == 4


def test_exported_grid_matches_the_mirror():
    k = consts()
    for C in bc.C_LIST + [5464, 8192]:
        for M in (1, 15, 16, 17, 511, 512, 513, 2736, 2737, 131684, 524365, 1 << 22):
            assert native().bn_bwd_reduce_blocks(M, C) == bc.reduce_blocks(M, C, k)[0], (M, C)


# ------------------------------------------------------------------------------ forward, exact
def _fwd_case(d, mode, dtype):
    r = None if mode == 0 else d.r
    rs, rb = (d.rscale, d.rbias) if mode == 2 else (None, None)
    cpu = (d.y, d.scale, d.bias, r, rs, rb)
    gpu = (act(d.y, dtype), vec(d.scale), vec(d.bias), act(r, dtype), vec(rs), vec(rb))
    return cpu, gpu


def _mask_bits(z):
    """The packed z > 0 of a stored [M, C] tensor: bit q of byte cg is channel 8*cg + q."""
    M, C = z.shape
    w = (1 << torch.arange(8, device=z.device)).to(torch.int32)
    return ((z > 0).reshape(M, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("C", bc.C_LIST, ids=lambda c: f"C{c}")
def test_forward_exact(C, dtype):
    k, u = consts(), apply_u()
    for M in sorted(set(bc.apply_rows(C, u, k).values())):    # asserts each M's edge
        d = bc.exact_inputs(C, M)
        for mode in (0, 1, 2):
            cpu, (y, sc, bi, r, rs, rb) = _fwd_case(d, mode, dtype)
            for relu in (True, False):
                ref, T = bc.ref_fwd(*cpu, relu)
                bc.assert_exact(ref, T * 2, stored=dtype)
                what = (C, M, mode, relu)
                z = native().bn_act_fwd(y, sc, bi, relu, r, rs, rb, None)
                assert same(z, ref), what
                # with the mask: same z, every byte the packed z > 0, nothing past M*C/8
                n = M * C // 8
                buf = torch.full((n + 256,), SENTINEL, dtype=torch.uint8, device=dev)
                zm = native().bn_act_fwd(y, sc, bi, relu, r, rs, rb, buf[:n].view(M, C // 8))
                assert torch.equal(zm, z), what
                assert torch.equal(buf[:n].view(M, C // 8), _mask_bits(z)), what
                assert bool((buf[n:] == SENTINEL).all()), what
                # streaming stores and loads: identical bits
                with nt_store(4 | 32):
                    buf2 = torch.full((n + 256,), SENTINEL, dtype=torch.uint8, device=dev)
                    zs = native().bn_act_fwd(y, sc, bi, relu, r, rs, rb, buf2[:n].view(M, C // 8))
                assert torch.equal(zs, z) and torch.equal(buf2, buf), what


# ------------------------------------------------------------------------------ backward apply, exact
def _apply_call(d, z, mode, relu, dtype):
    a = lambda t: act(t, dtype)
    two = mode == 2
    return native().bn_act_bwd_apply(
        a(d.dz), a(z), a(d.y), vec(d.mean), vec(d.invstd), vec(d.gamma), vec(d.sum_g),
        vec(d.sum_gx), d.count, relu, mode == 1, a(d.y2) if two else None,
        vec(d.mean2) if two else None, vec(d.invstd2) if two else None,
        vec(d.gamma2) if two else None, vec(d.sum_gx2) if two else None)


def _apply_ref(d, z, mode, relu):
    kw = dict(y2=d.y2, mean2=d.mean2, invstd2=d.invstd2, gamma2=d.gamma2,
              sum_gx2=d.sum_gx2) if mode == 2 else {}
    return bc.ref_apply(d.dz, z, d.y, d.mean, d.invstd, d.gamma, d.sum_g, d.sum_gx, d.count, relu,
                        **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("C", bc.C_LIST, ids=lambda c: f"C{c}")
def test_apply_exact(C, dtype):
    k, u = consts(), apply_u()
    for M in sorted(set(bc.apply_rows(C, u, k).values())):
        d = bc.exact_inputs(C, M)
        for mode in (0, 1, 2):
            for relu in (True, False):
                z = d.z if relu else d.zneg      # relu off: z must not be looked at
                o = _apply_ref(d, z, mode, relu)
                bc.assert_exact(o.dy, o.T * 32, stored=dtype)
                what = (C, M, mode, relu)
                dy, other = _apply_call(d, z, mode, relu, dtype)
                assert same(dy, o.dy), what
                if mode == 0:
                    assert other is None
                elif mode == 1:
                    assert same(other, o.g), what            # d(residual) = the masked g
                else:
                    bc.assert_exact(o.dy2, o.T2 * 32, stored=dtype)
                    assert same(other, o.dy2), what
                with nt_store(8 | 64):
                    dys, others = _apply_call(d, z, mode, relu, dtype)
                assert torch.equal(dys, dy), what
                assert other is None or torch.equal(others, other), what


# ------------------------------------------------------------------------------ backward reduce, exact
def _reduce_check(t, ref, C, M, relu, two, det, what):
    """One bn_act_bwd_reduce call on device operands ``t`` against float64 sums ``ref``: the sums,
    the accumulation into pre-filled gradients, and the replica slab's contract."""
    n, k = native(), consts()
    R = k.replicas
    fill = lambda seed: ((torch.arange(C, device=dev) * seed) % 17 - 8).float()
    dg, db, dg2, db2 = fill(3), fill(5), fill(7), fill(11)
    pre = [x.clone() for x in (dg, db, dg2, db2)]
    if det:   # the slab is not this mode's: a pattern must come back unchanged
        rep = ((torch.arange(3 * R * C, device=dev) % 13) - 6).float()
    else:     # a persistent zeroed slab is left zeroed
        rep = torch.zeros(3 * R * C, device=dev)
    rep0 = rep.clone()
    with deterministic(det):
        sg, sgx, sgx2 = n.bn_act_bwd_reduce(
            t.dz, t.z, t.y, t.mean, t.invstd, relu, t.y2 if two else None,
            t.mean2 if two else None, t.invstd2 if two else None, rep, dg, db, dg2, db2)
    assert same(sg, ref.sg) and same(sgx, ref.sgx), what
    assert torch.equal(rep, rep0), what
    assert same(db, pre[1].double().cpu() + ref.sg.cpu()), what
    assert same(dg, pre[0].double().cpu() + ref.sgx.cpu()), what
    if two:
        assert same(sgx2, ref.sgx2), what
        assert same(dg2, pre[2].double().cpu() + ref.sgx2.cpu()), what
        assert same(db2, pre[3].double().cpu() + ref.sg.cpu()), what
    else:
        assert sgx2 is None and torch.equal(dg2, pre[2]) and torch.equal(db2, pre[3]), what
    return sg, sgx, sgx2


def _reduce_exact(C, M, dtype, small=False, combos=None, dets=(False, True), on_gpu=False):
    k = consts()
    assert native().bn_bwd_reduce_blocks(M, C) == bc.reduce_blocks(M, C, k)[0]
    if on_gpu:   # the block-cap case: integers drawn on the device, reference in float64 there
        d = bc.exact_inputs(C, 64, small=True)     # the per-channel vectors depend on C alone
        assert small and M * d.term_max / d.term_step < bc.EXACT
        g = torch.Generator(device=dev)
        g.manual_seed(M)
        draw = lambda lo, hi: torch.randint(lo, hi + 1, (M, C), generator=g, device=dev,
                                            dtype=torch.int8)
        src = SimpleNamespace(y=draw(-2, 2), y2=draw(-2, 2), dz=draw(-1, 1), z=draw(0, 1) * 2)
        src.zneg = src.z
        where = dev
    else:
        d = bc.exact_inputs(C, M, small)
        assert bc.reduce_exact_bound(d) < bc.EXACT
        src, where = d, "cpu"
    vecs = {key: getattr(d, key).to(where) for key in ("mean", "invstd", "mean2", "invstd2")}
    for relu, two in combos or [(r, t) for r in (True, False) for t in (False, True)]:
        z = src.z if relu else src.zneg
        ref = bc.ref_reduce(src.dz, z, src.y, vecs["mean"], vecs["invstd"], relu,
                            src.y2 if two else None, vecs["mean2"], vecs["invstd2"])
        for s, a in ((ref.sg, ref.ag), (ref.sgx, ref.agx)) + (((ref.sgx2, ref.agx2),) if two else ()):
            bc.assert_exact(s, a / d.term_step)
        t = SimpleNamespace(dz=act(src.dz, dtype), z=act(z, dtype), y=act(src.y, dtype),
                            y2=act(src.y2, dtype), **{key: vec(v) for key, v in vecs.items()})
        for det in dets:
            _reduce_check(t, ref, C, M, relu, two, det, (C, M, relu, two, det))


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("C", bc.C_LIST, ids=lambda c: f"C{c}")
def test_reduce_exact_tails(C, dtype):
    for M in sorted(set(bc.reduce_rows(C, consts()).values())):   # asserts each M's tail
        _reduce_exact(C, M, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("name", ["budget", "budget_2pass", "floor", "block_cap"])
def test_reduce_exact_grid_limits(name, dtype):
    k = consts()
    _, C, M, small = next(c for c in bc.cap_cases(k) if c[0] == name)    # asserts the mirror
    G = native().bn_bwd_reduce_blocks(M, C)
    rpb = bc.row_map(C, k)[1]
    assert G < bc.cdiv(M, rpb * k.row_iters)          # a limit binds, whichever it is, and ...
    want = {"budget": k.atomic_budget // (3 * C), "budget_2pass": k.atomic_budget // (3 * C),
            "floor": k.min_blocks, "block_cap": k.reduce_blocks}[name]
    assert G == want                                  # ... it is the one the case is named after
    if name == "floor":
        assert k.atomic_budget // (3 * C) < k.min_blocks
    big = name == "block_cap"
    _reduce_exact(C, M, dtype, small, combos=[(True, True), (False, False)] if big else None,
                  on_gpu=big)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("name", ["sum16_tails", "chunk_sums"])
def test_reduce_exact_deterministic_collect(name, dtype):
    k = consts()
    _, C, M = next(c for c in bc.det_cases(k) if c[0] == name)           # asserts the mirror
    G = native().bn_bwd_reduce_blocks(M, C)
    if name == "sum16_tails":
        assert G <= 4 * k.det_chunk_rows and min(bc.rows_sum16_loops(G)) >= 1 and G % 16
    else:
        assert G > 4 * k.det_chunk_rows and G % k.det_chunk_rows
    _reduce_exact(C, M, dtype, combos=[(True, True), (False, False)])


# ------------------------------------------------------------------------------ random data
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", bc.RANDOM_CASES, ids=lambda c: c[0])
def test_random_forward_and_apply(case, dtype):
    name, C, M, offset = case
    d = bc.random_inputs(name, C, M, offset, dtype)
    if offset and dtype == torch.float32:
        q = (d.mean.abs() * d.invstd).median().item()
        assert 300 < q < 3000, q                      # |mean| * invstd about 1000
    a = lambda t: act(t, dtype)
    for relu in (True, False):
        for mode in (0, 1, 2):
            r = None if mode == 0 else (d.r if mode == 1 else d.y2)
            rs, rb = (d.rscale, d.rbias) if mode == 2 else (None, None)
            ref, T = bc.ref_fwd(d.y, d.scale, d.bias, r, rs, rb, relu)
            z = native().bn_act_fwd(a(d.y), vec(d.scale), vec(d.bias), relu, a(r), vec(rs), vec(rb),
                                    None)
            q = bc.worst(z.cpu(), ref, bc.elementwise_bound(ref, T, dtype))
            print(f"fwd {name} {bc.DT_ID[dtype]} mode {mode} relu {relu}: worst/bound {q:.3f}")
            assert q <= 1, ("fwd", mode, relu, q)
            o = _apply_ref(d, d.z, mode, relu)
            dy, other = _apply_call(d, d.z, mode, relu, dtype)
            q = bc.worst(dy.cpu(), o.dy, bc.elementwise_bound(o.dy, o.T, dtype))
            print(f"apply {name} {bc.DT_ID[dtype]} mode {mode} relu {relu}: worst/bound {q:.3f}")
            assert q <= 1, ("apply", mode, relu, q)
            if mode == 1:
                assert same(other, o.g.to(dtype).double())
            if mode == 2:
                q = bc.worst(other.cpu(), o.dy2, bc.elementwise_bound(o.dy2, o.T2, dtype))
                print(f"apply2 {name} {bc.DT_ID[dtype]} relu {relu}: worst/bound {q:.3f}")
                assert q <= 1, ("apply2", relu, q)


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", bc.RANDOM_CASES, ids=lambda c: c[0])
def test_random_reduce(case, dtype):
    name, C, M, offset = case
    k = consts()
    d = bc.random_inputs(name, C, M, offset, dtype)
    a = lambda t: act(t, dtype)
    args = (a(d.dz), a(d.z), a(d.y), vec(d.mean), vec(d.invstd), True, a(d.y2), vec(d.mean2),
            vec(d.invstd2))
    ref = bc.ref_reduce(d.dz, d.z, d.y, d.mean, d.invstd, True, d.y2, d.mean2, d.invstd2)
    for det in (False, True):
        chain = bc.reduce_chain(M, C, k, det)
        with deterministic(det):
            out = native().bn_act_bwd_reduce(*args)
            again = native().bn_act_bwd_reduce(*args) if det else None
        for key, o, r, mags in (("sg", out[0], ref.sg, ref.ag), ("sgx", out[1], ref.sgx, ref.agx),
                                ("sgx2", out[2], ref.sgx2, ref.agx2)):
            q = bc.worst(o.cpu(), r, bc.reduce_bound(mags, chain))
            print(f"reduce {name} {bc.DT_ID[dtype]} det {det} {key}: chain {chain} worst/bound {q:.3f}")
            assert q <= 1, (key, det, q)
        if det:   # a fixed order of additions: the same bits every time
            assert all(torch.equal(x, y) for x, y in zip(out, again))


# ------------------------------------------------------------------------------ bn_finalize, replicas
@pytest.mark.parametrize("count", [1, 4096])
@pytest.mark.parametrize("C", [8, 200, 2056], ids=lambda c: f"C{c}")
def test_finalize_replica_route(C, count):
    n, R = native(), native().STAT_REPLICAS
    d = bc.finalize_inputs(C, count, R)
    o = bc.ref_finalize(d.psum, d.psq, count, d.shift, d.gamma, d.beta, bc.EPS)
    neg = bc.NEG_VAR_CHANNEL
    assert o.raw_var[neg].item() < 0 and o.var[neg].item() == 0
    psum, psq = d.psum.to(dev), d.psq.to(dev)
    # running statistics and num_batches_tracked absent, the slab kept
    mean, invstd, scale, bias = n.bn_finalize(psum, psq, count, vec(d.shift), vec(d.gamma),
                                              vec(d.beta), None, None, 0.1, bc.EPS, False, None)
    assert torch.equal(psum.cpu(), d.psum) and torch.equal(psq.cpu(), d.psq)
    assert torch.allclose(mean.double().cpu(), o.mean, rtol=1e-5, atol=1e-5)
    q = bc.worst(invstd.cpu(), o.invstd, o.invstd_tol)
    print(f"finalize C {C} count {count}: invstd worst/bound {q:.3f}")
    assert q <= 1
    assert invstd[neg].item() == pytest.approx(bc.EPS ** -0.5, rel=8 * bc.U24)
    # scale and bias are one and two fp32 operations on the outputs just checked
    m64, s64 = mean.double().cpu(), scale.double().cpu()
    assert bool(((s64 - d.gamma.double() * invstd.double().cpu()).abs() <= 2 * bc.U24 * s64.abs()).all())
    tol = 4 * bc.U24 * (d.beta.double().abs() + (m64 * s64).abs())
    assert bool(((bias.double().cpu() - (d.beta.double() - m64 * s64)).abs() <= tol).all())
    # with running statistics: var = 0 in the clamped channel, unbias = 1 for count = 1; the slab
    # is cleared
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    nbt = torch.tensor(4, dtype=torch.int64, device=dev)
    out = n.bn_finalize(psum, psq, count, vec(d.shift), vec(d.gamma), vec(d.beta), rm, rv, 0.1,
                        bc.EPS, True, nbt)
    assert all(torch.equal(x, y) for x, y in zip(out, (mean, invstd, scale, bias)))
    assert int(nbt) == 5 and not psum.any() and not psq.any()
    unbias = count / (count - 1) if count > 1 else 1.0
    assert torch.allclose(rm.double().cpu(), 0.1 * o.mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rv.double().cpu(), 0.9 + 0.1 * o.var * unbias, rtol=1e-5, atol=1e-6)
    assert rv[neg].item() == pytest.approx(0.9, rel=4 * bc.U24)


# ------------------------------------------------------------------------------ U = 4
def test_u4_instantiations():
    """The U = 4 instantiations of the two apply kernels are chosen when the library is loaded, so
    they run in a fresh interpreter: the smallest exact forward and apply cases (whose tiles are
    derived from bn_apply_u(), now 4) and the assertion that U = 4 is in effect."""
    if os.environ.get(CHILD):
        return      # this is the child
    env = dict(os.environ, MIPIPE_BN_U="4")
    env[CHILD] = "1"
    select = ("test_apply_u_in_effect or ((test_forward_exact or test_apply_exact) and "
              "(C8- or C40-))")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m",
                        "gpu", "-p", "no:cacheprovider", "-k", select],
                       env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert "9 passed" in p.stdout and "skipped" not in p.stdout, tail
