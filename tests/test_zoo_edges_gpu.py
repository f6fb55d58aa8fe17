"""vision.hip and the max-pool pair of pool.hip past their launch edges: grid caps, unroll tails,
row splits, grid-stride second trips, pool geometry, ties and NaN.

The unit tests of test_zoo_gpu.py / test_fp32_gpu.py use shapes at which every launch collapses
to its trivial case (one block pass, one split, one grid-stride trip).  Here every shape is derived
from the launch constants the extension exports (``V8_ROW_U`` ... ``EW_GRID_BLOCKS``, next to
``STAT_REPLICAS``) and each test asserts, from the launcher's own formula, that the shape crosses
the edge it is meant to cross.

Reductions are tested with integer-valued data: every product, every partial sum and the result
are exactly representable in fp32 (and in bf16 where bf16 is stored), so any summation order gives
the same bits and one dropped or repeated element moves the answer by a whole unit.  Each such
test first asserts the exactness condition on its float64 reference (``_assert_exact``); the
comparison is then ``torch.equal``.  Elementwise passes use random data and the bounds of the
existing tests (1e-4 fp32, 1e-2 bf16, relative to the output magnitude).

Run on an MI355X:  python -m pytest tests/test_zoo_edges_gpu.py -m gpu
"""
import itertools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from mipipe.ops import _ref
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu
dev = "cuda"
ACT = {"none": 0, "relu": 1, "relu6": 2}
DTYPES = [torch.bfloat16, torch.float32]
TOL = {torch.bfloat16: 1e-2, torch.float32: 1e-4}  # test_zoo_gpu.py / test_fp32_gpu.py
EXACT = 2 ** 24  # integers below this magnitude are exact in fp32
DT_ID = {torch.bfloat16: "bf16", torch.float32: "fp32"}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(1234)


_SLOT = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared():
    yield
    _SLOT.clear()


def shared(name, key, make):
    """Inputs and float64 reference of one case, made once and shared by the dtypes that run it
    (consecutive parameters); one slot per test, never modified by its users."""
    if name not in _SLOT or _SLOT[name][0] != key:
        _SLOT.pop(name, None)
        _SLOT[name] = (key, make())
    return _SLOT[name][1]


def consts():
    n = native()
    return SimpleNamespace(row_u=n.V8_ROW_U, apply_u=n.V8_APPLY_U, reduce_blocks=n.V8_REDUCE_BLOCKS,
                           apply_blocks=n.V8_APPLY_BLOCKS, chan_blocks=n.CHAN_GRID_BLOCKS,
                           grid_for=n.GRID_FOR_BLOCKS, ew_grid=n.EW_GRID_BLOCKS,
                           replicas=n.STAT_REPLICAS)


def cdiv(a, b):
    return -(-a // b)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def pm1(*shape):
    """float64 values in {-1, +1}: never 0, so every element counts."""
    return (torch.randint(0, 2, shape, device=dev) * 2 - 1).double()


def choice(values, *shape):
    v = torch.tensor(values, dtype=torch.float64, device=dev)
    return v[torch.randint(0, len(values), shape, device=dev)]


def act_z(act, *shape):
    """An activation OUTPUT whose mask keeps about half: relu 0 | 2, relu6 0 | 3 | 6 (0 and 6 are
    what a clamped output really holds, and they sit exactly on the mask's comparisons)."""
    if act == "none":
        return None
    return choice([0.0, 2.0] if act == "relu" else [0.0, 3.0, 3.0, 6.0], *shape)


def cast(t, dtype):
    return None if t is None else t.to(dtype)


def _assert_exact(ref, abs_terms, stored=None):
    """The condition under which a zero tolerance is right: the reference is representable in
    fp32 (and in ``stored`` when the kernel stores bf16) and, per output, the sum of the terms'
    magnitudes stays below 2**24, so every partial sum in any order is an exact fp32 integer
    (or, for the average pools, an exact multiple of a power of two)."""
    assert torch.equal(ref, ref.float().double())
    if stored == torch.bfloat16:
        assert torch.equal(ref, ref.to(torch.bfloat16).double())
    bound = abs_terms.max().item() if torch.is_tensor(abs_terms) else abs_terms
    assert bound < EXACT, bound


# ------------------------------------------------------------------- BatchNorm, any C: shapes
V8_C = [8, 40, 96, 1000, 2048]   # tpr = 1 | idle threads (256 % 5) | 12 | idle (256 % 125) | 256
GENERIC_C = [58, 2056]           # C % 8 != 0; C % 8 == 0 but above bn_v8's 2048


def is_v8(C):  # vision.hip: bn_v8
    return C % 8 == 0 and C <= 2048


def rpb_of(C):  # rows per block pass of the v8 kernels: rpb = 256 / tpr, tpr = C / 8
    return 256 // (C // 8)


def reduce_rows(C, kind):
    """M for chan_stats / bn_generic_bwd_reduce, with the edge it crosses asserted from the
    launchers (vision.hip: v8_grid and the r0 loop of chan_stats_v8_kernel /
    bn_generic_bwd_reduce_v8_kernel; chan_grid and the row loop of the generic kernels)."""
    k = consts()
    if kind == "one":
        return 1
    if is_v8(C):
        rpb = rpb_of(C)
        if kind == "sub_block":          # fewer rows than one block pass
            return max(1, rpb - 1)
        slots = {"past_cap": 2, "second_trip": k.row_u + 1}[kind]
        M = k.reduce_blocks * rpb * slots + rpb // 2 + 1
        blocks = max(1, min(cdiv(M, rpb), k.reduce_blocks))       # v8_grid
        stride = blocks * rpb
        trips = cdiv(M, k.row_u * stride)                         # outer trips of block 0
        assert blocks == k.reduce_blocks                          # the grid is at its cap
        assert trips == (1 if kind == "past_cap" else 2)
        # `slots` unroll slots are full; the next holds rows of block 0 only (rpb//2 + 1 of its
        # rpb), the rest none: the clamp to M-1 and its `break` run in every other block
        assert 0 < M - slots * stride <= rpb and slots % k.row_u != 0
        return M
    bx = cdiv(C, 64)
    cap = max(1, k.chan_blocks // bx)                             # chan_grid
    if kind == "small":
        return 37
    assert kind == "chan_cap"
    M = cap * 64 + 5
    assert cdiv(M, 64) > cap and cdiv(M, cap * 4) > 1             # capped grid, several row trips
    return M


REDUCE_CASES = [(C, kind) for C in V8_C for kind in ("one", "sub_block", "past_cap", "second_trip")]
REDUCE_CASES += [(58, "one"), (58, "chan_cap"), (2056, "small"), (2056, "chan_cap")]


def apply_rows(C, kind):
    """M for affine_act / bn_generic_bwd_apply (vision.hip: v8_tiles and the r0 loop of the
    *_v8 apply kernels; grid_for and the grid-stride loop of the generic ones)."""
    k = consts()
    if kind == "one":
        return 1
    if kind == "small":
        return 5
    if is_v8(C):
        assert kind == "second_trip"
        rpb = rpb_of(C)
        tile = rpb * k.apply_u
        M = k.apply_blocks * tile + rpb + 1
        blocks = max(1, min(cdiv(M, tile), k.apply_blocks))       # v8_tiles
        assert blocks == k.apply_blocks and cdiv(M, blocks * tile) == 2
        # second trip: block 0's first unroll slot is full, its second holds a single row
        assert M - blocks * tile - rpb == 1 and k.apply_u == 2
        return M
    assert kind == "grid_cap"
    M = (k.grid_for * 256) // C + 2
    assert cdiv(M * C, 256) > k.grid_for and M * C <= 2 * k.grid_for * 256   # grid_for: 2 trips
    return M


APPLY_CASES = [(C, kind) for C in V8_C for kind in ("one", "second_trip")]
APPLY_CASES += [(58, "grid_cap"), (2056, "small")]


def _ids(cases):
    return ["-".join(DT_ID.get(v, str(v)) for v in c) for c in cases]


# ------------------------------------------------------------------- exact reductions
def _chan_stats_case(M, C):
    y = pm1(M, C)
    shift = choice([-1.0, 0.0, 1.0], C)
    ps, pq = _ref.chan_stats(y, shift)
    d = y - shift
    _assert_exact(ps, d.abs().sum(0))
    _assert_exact(pq, (d * d).sum(0))
    return y, shift, ps, pq


_CS = [c + (dt,) for c in REDUCE_CASES for dt in DTYPES]


@pytest.mark.parametrize("C,kind,dtype", _CS, ids=_ids(_CS))
def test_chan_stats_exact(C, kind, dtype):
    M = reduce_rows(C, kind)
    y64, shift, psr, pqr = shared("chan_stats", (C, kind), lambda: _chan_stats_case(M, C))
    y = y64.to(dtype)
    ps, pq = native().chan_stats(y, shift.float())
    assert ps.shape[0] == consts().replicas            # replica rows, summed by bn_finalize
    assert torch.equal(ps.double().sum(0, keepdim=True), psr)
    assert torch.equal(pq.double().sum(0, keepdim=True), pqr)
    # y = +-1, shift = 0: the sum of squares is the number of rows visited, in every channel
    ps, pq = native().chan_stats(y, torch.zeros(C, device=dev))
    assert torch.equal(pq.double().sum(0), torch.full((C,), float(M), dtype=torch.float64, device=dev))
    assert torch.equal(ps.double().sum(0), y64.sum(0))


def _bwd_reduce_case(M, C, act):
    dz, y, z = pm1(M, C), pm1(M, C), act_z(act, M, C)
    mean = choice([-1.0, 0.0, 1.0], C)
    invstd = choice([0.5, 1.0, 2.0], C)                # powers of two
    sg, sgx = _ref.bn_generic_bwd_reduce(dz, z, y, mean, invstd, act)
    keep = None if z is None else _ref.act_keep(z, act)
    g = dz if keep is None else dz * keep
    if keep is not None and M >= 64:
        assert 0.3 < keep.double().mean().item() < 0.7
    _assert_exact(sg, g.abs().sum(0))
    _assert_exact(sgx, (g * (y - mean) * invstd).abs().sum(0))
    return dz, z, y, mean, invstd, sg, sgx


_BR = [c + (act, dt) for c in REDUCE_CASES for act in ACT for dt in DTYPES]


@pytest.mark.parametrize("C,kind,act,dtype", _BR, ids=_ids(_BR))
def test_bn_generic_bwd_reduce_exact(C, kind, act, dtype):
    M = reduce_rows(C, kind)
    dz, z, y, mean, invstd, sgr, sgxr = shared("bwd_reduce", (C, kind, act),
                                               lambda: _bwd_reduce_case(M, C, act))
    sg, sgx = native().bn_generic_bwd_reduce(dz.to(dtype), cast(z, dtype), y.to(dtype), mean.float(),
                                             invstd.float(), ACT[act])
    assert torch.equal(sg.double(), sgr)
    assert torch.equal(sgx.double(), sgxr)


# ------------------------------------------------------------------- apply passes (elementwise)
def _check_apply(out, ref, dtype, C, what):
    """The existing bound relative to the output magnitude and, for the last rows (the partial
    unroll slot / the last grid-stride trip), the same bound relative to each element's own
    magnitude, so a wrong tail cannot hide behind a large maximum elsewhere."""
    tol = TOL[dtype]
    assert out.dtype == dtype and out.shape == ref.shape
    e = rel_err(out, ref)
    tail = 2 * (rpb_of(C) if is_v8(C) else 256)
    o, r = out.double()[-tail:], ref[-tail:]
    worst = ((o - r).abs() / r.abs().clamp_min(1e-30)).max().item()
    print(f"{what}: rel_err {e:.3e}, worst tail element {worst:.3e} (bound {tol:g})")
    assert e < tol
    assert bool(((o - r).abs() <= tol * r.abs()).all())


def _signs(*shape):
    return (torch.randint(0, 2, shape, device=dev) * 2 - 1).float()


_AP = [c + (act, dt) for c in APPLY_CASES for act in ACT for dt in DTYPES]


@pytest.mark.parametrize("C,kind,act,dtype", _AP, ids=_ids(_AP))
def test_affine_act_tail(C, kind, act, dtype):
    """|y * scale| >= 0.25 and |bias| <= 0.125 keep every pre-activation at least 0.125 from zero
    (no cancellation, no sign flip between fp32 and float64), so the per-element bound on the tail
    is meaningful; mixed signs make ReLU mask half, |y * scale| up to 12 makes ReLU6 clamp some."""
    M = apply_rows(C, kind)
    y = ((torch.rand(M, C, device=dev) * 7.5 + 0.5) * _signs(M, C)).to(dtype)
    scale = (torch.rand(C, device=dev) + 0.5) * _signs(C)
    bias = (torch.rand(C, device=dev) - 0.5) * 0.25
    z = native().affine_act(y, scale, bias, ACT[act])
    ref = _ref.affine_act(y.double(), scale.double(), bias.double(), act)
    _check_apply(z, ref, dtype, C, "affine_act")


@pytest.mark.parametrize("C,kind,act,dtype", _AP, ids=_ids(_AP))
def test_bn_generic_bwd_apply_tail(C, kind, act, dtype):
    """Magnitudes chosen so that g - sum_g/n - xhat * sum_gx/n never comes near zero: |g| in
    [1, 2) where the mask passes, |sum_g/n| in [1/16, 1/8], |xhat * sum_gx/n| <= 0.03 (|xhat| <=
    3.75), hence |v| >= 0.03 under the mask and >= 0.84 elsewhere; the eval form (no sums) gives
    exact zeros under the mask on both sides."""
    M = apply_rows(C, kind)
    dz = ((torch.rand(M, C, device=dev) + 1.0) * _signs(M, C)).to(dtype)
    y = (torch.rand(M, C, device=dev) * 4 - 2).to(dtype)
    z = cast(act_z(act, M, C), dtype)
    mean = torch.rand(C, device=dev) - 0.5
    invstd = torch.rand(C, device=dev) + 0.5
    gamma = (torch.rand(C, device=dev) + 0.5) * _signs(C)
    sum_g = (torch.rand(C, device=dev) + 1.0) * 0.0625 * _signs(C) * M
    sum_gx = (torch.rand(C, device=dev) + 1.0) * 0.004 * _signs(C) * M
    d = lambda t: None if t is None else t.double()  # noqa: E731
    dy = native().bn_generic_bwd_apply(dz, z, y, mean, invstd, gamma, sum_g, sum_gx, M, ACT[act])
    ref = _ref.bn_generic_bwd_apply(d(dz), d(z), d(y), d(mean), d(invstd), d(gamma), d(sum_g),
                                    d(sum_gx), M, act)
    _check_apply(dy, ref, dtype, C, "bn_generic_bwd_apply")
    dy = native().bn_generic_bwd_apply(dz, z, y, mean, invstd, gamma, None, None, M, ACT[act])
    ref = _ref.bn_generic_bwd_apply(d(dz), d(z), d(y), d(mean), d(invstd), d(gamma), None, None, M,
                                    act)
    _check_apply(dy, ref, dtype, C, "bn_generic_bwd_apply (eval)")


# ------------------------------------------------------------------- weight-grad row splits
def dw_split(C, taps, N, Ho, Wo):
    """(by, rows_per, rows of the last split) of vision.hip's dwconv_wgrad launcher."""
    lanes = 256 // (C // 8)
    P, R = N * Ho * Wo, N * Ho
    splits = max(1, 2048 // taps)
    splits = min(splits, max(1, P // (lanes * 32)))
    splits = min(splits, R, 65535)
    rows_per = cdiv(R, splits)
    by = cdiv(R, rows_per)
    return by, rows_per, R - (by - 1) * rows_per


def gconv_split(Co, Cig, taps, R):
    """The same of the generic gconv_wgrad launcher (R = N * Ho rows, >= 4 rows per split)."""
    bx = cdiv(Co * Cig, 256)
    splits = max(1, 2048 // max(1, bx * taps))
    splits = min(splits, max(1, R // 4), 65535)
    rows_per = cdiv(R, splits)
    by = cdiv(R, rows_per)
    return by, rows_per, R - (by - 1) * rows_per


def _wgrad_case(N, Ho, Wo, Ci, Co, k, s, p, groups, act):
    H = (Ho - 1) * s[0] + k[0] - 2 * p[0]
    W = (Wo - 1) * s[1] + k[1] - 2 * p[1]
    dy, x, z = pm1(N, Ho, Wo, Co), pm1(N, H, W, Ci), act_z(act, N, Ho, Wo, Co)
    dw, db = _ref.gconv_wgrad(dy, x, k[0], k[1], s, p, groups, z, act)
    # |dy * x| <= 1: a weight element sums at most one term per output position, the bias
    # gradient exactly one, so the number of positions bounds the terms' magnitudes
    _assert_exact(dw, N * Ho * Wo)
    _assert_exact(db, N * Ho * Wo)
    return dy, x, z, dw, db


def _run_wgrad(case, dtype, act, name):
    N, Ho, Wo, Ci, Co, k, s, p, groups = case
    dy64, x64, z64, dwr, dbr = shared(name, (case, act), lambda: _wgrad_case(*case, act))
    dy, x, z = dy64.to(dtype), x64.to(dtype), cast(z64, dtype)
    args = (dy, x, k[0], k[1], list(s), list(p), groups, z, ACT[act])
    dw, db = native().gconv_wgrad(*args, None, None, True)          # zeroed outputs
    assert torch.equal(dw.double(), dwr) and torch.equal(db.double(), dbr)
    # accumulation into the flat-gradient views: integer constants, still exact
    acc, accb = torch.full_like(dw, 3.0), torch.full_like(db, 5.0)
    native().gconv_wgrad(*args, acc, accb, False)
    assert torch.equal(acc.double(), dwr + 3) and torch.equal(accb.double(), dbr + 5)


_DW = [(C, k, s, act, dt) for C in (8, 40, 96, 2048) for k in (3, 5) for s in (1, 2)
       for act in ("none", "relu6") for dt in DTYPES]


@pytest.mark.parametrize("C,k,s,act,dtype", _DW, ids=_ids(_DW))
def test_dwconv_wgrad_splits_exact(C, k, s, act, dtype):
    """dwconv_wgrad_v8_kernel with blockIdx.y > 0, a short last split and the cross-block atomics
    on dw and dbias: the smallest square output (N = 2) with >= 3 splits and R % rows_per != 0."""
    N = 2
    Ho = next(h for h in range(2, 400) if dw_split(C, k * k, N, h, h)[0] >= 3
              and dw_split(C, k * k, N, h, h)[2] < dw_split(C, k * k, N, h, h)[1])
    by, rows_per, last = dw_split(C, k * k, N, Ho, Ho)
    assert by >= 3 and 0 < last < rows_per and (N * Ho) % rows_per != 0
    _run_wgrad((N, Ho, Ho, C, C, (k, k), (s, s), (k // 2, k // 2), C), dtype, act, "dw_wgrad")


# Ci, Co, (kh, kw), (sh, sw), (ph, pw), groups
GCONV_WGRAD = {"resnext32x4d": (128, 128, (3, 3), (1, 1), (1, 1), 32),
               "dw58_s2": (58, 58, (3, 3), (2, 2), (1, 1), 58),
               "inception1x7": (64, 48, (1, 7), (1, 1), (0, 3), 1)}
_GW = [(n, rows, dt) for n in GCONV_WGRAD for rows in ("short_last", "single") for dt in DTYPES]


@pytest.mark.parametrize("name,rows,dtype", _GW, ids=_ids(_GW))
def test_gconv_wgrad_splits_exact(name, rows, dtype):
    Ci, Co, k, s, p, groups = GCONV_WGRAD[name]
    taps, Cig = k[0] * k[1], Ci // groups
    if rows == "single":               # R < 4: one split, blockIdx.y == 0 only
        N, Ho = 1, 3
        assert gconv_split(Co, Cig, taps, N * Ho)[0] == 1
    else:
        N = 2
        Ho = next(h for h in range(2, 200) if gconv_split(Co, Cig, taps, N * h)[0] >= 3
                  and (N * h) % gconv_split(Co, Cig, taps, N * h)[1] != 0)
        by, rows_per, last = gconv_split(Co, Cig, taps, N * Ho)
        assert by >= 3 and 0 < last < rows_per
    _run_wgrad((N, Ho, Ho + 2, Ci, Co, k, s, p, groups), dtype, "relu6", "g_wgrad")


# ------------------------------------------------------------------- grid-stride second trips
def _second_trip_side(per_pixel, cap, N=2):
    """Smallest square side with N * side^2 * per_pixel work items above cap * 256 (one more
    grid-stride trip for some threads, not for all)."""
    side = next(h for h in range(1, 4096) if N * h * h * per_pixel > cap * 256)
    assert cap * 256 < N * side * side * per_pixel < 2 * cap * 256
    return side


def _conv_case(N, H, C, k, act):
    """Depthwise k x k, stride 1, 'same' padding: x, w = +-1, integer bias; sums <= k*k + 2."""
    x, w = pm1(N, H, H, C), pm1(C, k, k, 1)
    b = choice([-2.0, -1.0, 0.0, 1.0, 2.0], C)
    s, p = (1, 1), (k // 2, k // 2)
    y = _ref.gconv_fwd(x, w, s, p, C, b, act)
    assert k * k + 2 <= 256
    _assert_exact(y, k * k + 2, torch.bfloat16)
    dy = pm1(N, H, H, C)
    dx = _ref.gconv_dgrad(dy, w, (N, H, H, C), s, p, C, y, act)
    _assert_exact(dx, k * k, torch.bfloat16)
    assert 0.1 < _ref.act_keep(y, act).double().mean().item() < 0.9
    return x, w, b, y, dy, dx


_GS = [(C, k, dt) for C, k in ((58, 3), (8, 3), (8, 5)) for dt in DTYPES]


@pytest.mark.parametrize("C,k,dtype", _GS, ids=_ids(_GS))
def test_conv_grid_stride_second_trip_exact(C, k, dtype):
    """gconv_fwd / gconv_dgrad (C = 58), dwconv3_fwd_v8 (C = 8, 3x3), dwconv_fwd_v8 (5x5) and
    dwconv_dgrad_v8 with more work items than grid_for's cap covers in one pass; ReLU6 fused in
    forward, its mask read from z in the data-grad."""
    N, act = 2, "relu6"
    H = _second_trip_side(C // 8 if C % 8 == 0 else C, consts().grid_for, N)
    x, w, b, yr, dy, dxr = shared("conv_trip", (C, k), lambda: _conv_case(N, H, C, k, act))
    s, p = [1, 1], [k // 2, k // 2]
    y = native().gconv_fwd(x.to(dtype), w.to(dtype), s, p, C, b.float(), ACT[act])
    assert y.dtype == dtype and torch.equal(y.double(), yr)
    dx = native().gconv_dgrad(dy.to(dtype), w.to(dtype), [N, H, H, C], s, p, C, y, ACT[act])
    assert torch.equal(dx.double(), dxr)


def _avg_case(N, H, W, C, k, s, p, exact):
    if exact:
        x = pm1(N, H, W, C)
    else:
        x = torch.randn(N, H, W, C, device=dev).to(torch.bfloat16).double()
    y = _ref.avgpool2d_fwd(x, k, s, p)
    dy = pm1(*y.shape) if exact else torch.randn(*y.shape, device=dev).to(torch.bfloat16).double()
    dx = _ref.avgpool2d_bwd(dy, (N, H, W, C), k, s, p)
    if exact:  # k*k is a power of two: sums of +-1 scaled by 2^-2 / 2^-4
        assert k in (2, 4)
        _assert_exact(y, k * k, torch.bfloat16)
        _assert_exact(dx, k * k, torch.bfloat16)
    return x, y, dy, dx


def _run_avgpool(case, dtype, name):
    N, H, W, C, k, s, p = case
    exact = k in (2, 4)
    x, yr, dy, dxr = shared(name, case, lambda: _avg_case(*case, exact))
    y = native().avgpool2d_fwd(x.to(dtype), k, s, p)
    dx = native().avgpool2d_bwd(dy.to(dtype), [N, H, W, C], k, s, p)
    assert y.shape == yr.shape and y.dtype == dtype and dx.shape == dxr.shape
    if exact:
        assert torch.equal(y.double(), yr) and torch.equal(dx.double(), dxr)
    else:
        assert rel_err(y, yr) < TOL[dtype] and rel_err(dx, dxr) < TOL[dtype]


_AT = [(k, s, p, C, dt) for k, s, p, C in ((2, 2, 0, 64), (4, 2, 1, 58), (3, 2, 1, 64))
       for dt in DTYPES]


@pytest.mark.parametrize("k,s,p,C,dtype", _AT, ids=_ids(_AT))
def test_avgpool2d_grid_stride_second_trip(k, s, p, C, dtype):
    N = 2
    Ho = _second_trip_side(C, consts().grid_for, N)          # forward: N * Ho * Wo * C items
    H = (Ho - 1) * s + k - 2 * p + (1 if s > 1 else 0)       # one more row / column than used
    assert (H + 2 * p - k) // s + 1 == Ho
    assert N * H * H * C > consts().grid_for * 256           # backward: N * H * W * C items
    _run_avgpool((N, H, H, C, k, s, p), dtype, "avg_trip")


def _maxpool_dev_ref(x64, k, s, p, ceil):
    xr = x64.permute(0, 3, 1, 2).requires_grad_()
    y = F.max_pool2d(xr, k, s, p, ceil_mode=ceil)
    dy = torch.randint(-4, 5, tuple(y.shape), device=x64.device).double()
    y.backward(dy)
    return (y.detach().permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1).contiguous(),
            xr.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids([(d,) for d in DTYPES]))
def test_maxpool_grid_stride_second_trip(dtype):
    """maxpool_fwd / maxpool_bwd with more 8-channel groups than ew_grid's cap covers in one pass
    (3x3, stride 1, pad 1, C = 8); integer dy makes the backward sums exact."""
    N, C, k, s, p = 2, 8, 3, 1, 1
    H = _second_trip_side(1, consts().ew_grid, N)
    x = torch.randn(N, H, H, C, device=dev).to(dtype)
    yr, dy, dxr = _maxpool_dev_ref(x.double(), k, s, p, False)
    y, idx = native().maxpool_fwd(x, k, s, p, False)
    assert torch.equal(y.double(), yr)
    dx = native().maxpool_bwd_impl(dy.to(dtype), idx, [N, H, H, C], k, s, p)
    assert torch.equal(dx.double(), dxr)


# ------------------------------------------------------------------- pool geometry, ties, NaN
def _maxpool_cpu_ref(x, k, s, p, ceil, dy=None):
    """torch's CPU float64 max-pool of NHWC ``x`` and its gradient for ``dy`` (made here as small
    integers when not given): the first maximum in scan order takes the gradient."""
    xr = x.detach().double().cpu().permute(0, 3, 1, 2).requires_grad_()
    y = F.max_pool2d(xr, k, s, p, ceil_mode=ceil)
    if dy is None:
        dy = torch.randint(-4, 5, tuple(y.shape)).double().permute(0, 2, 3, 1).contiguous()
    y.backward(dy.double().cpu().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), dy, xr.grad.permute(0, 2, 3, 1)


def _maxpool_both(x, k, s, p, ceil, dy=None):
    yr, dy, dxr = _maxpool_cpu_ref(x, k, s, p, ceil, dy)
    y, idx = native().maxpool_fwd(x, k, s, p, ceil)
    dx = native().maxpool_bwd_impl(dy.to(x.dtype).to(dev), idx, list(x.shape), k, s, p)
    return y.double().cpu(), yr, dx.double().cpu(), dxr, dy


POOL_GEO = [(k, s, p) for k in (2, 3) for s in (1, 2, 3) for p in (0, 1)]   # 2p <= k throughout
POOL_HW = [(1, 1), (2, 5), (7, 4), (13, 14)]
_MP = [(C, ceil, dt) for C in (8, 64) for ceil in (False, True) for dt in DTYPES]


@pytest.mark.parametrize("C,ceil,dtype", _MP, ids=_ids(_MP))
def test_maxpool_geometry_sweep(C, ceil, dtype):
    bad, ran = [], 0
    for (k, s, p), (H, W) in itertools.product(POOL_GEO, POOL_HW):
        if min(H, W) + 2 * p < k:      # no output: the entry raises (test_binding_checks_gpu.py)
            continue
        x = torch.randn(2, H, W, C).to(dtype).to(dev)
        y, yr, dx, dxr, _ = _maxpool_both(x, k, s, p, ceil)
        ran += 1
        if y.shape != yr.shape or not torch.equal(y, yr) or not torch.equal(dx, dxr):
            bad.append((k, s, p, H, W))
    assert ran == 39 and not bad, bad   # 48 combinations, 9 with an input below the window


@pytest.mark.parametrize("C,dtype", [(C, dt) for C in (8, 64) for dt in DTYPES],
                         ids=_ids([(C, dt) for C in (8, 64) for dt in DTYPES]))
def test_maxpool_ties(C, dtype):
    """Whole windows of equal values, and three-valued inputs where most windows tie: the output
    is the value, the gradient goes to the first maximum in scan order (kh, then kw)."""
    N, H, W = 2, 13, 14
    hh, ww = torch.arange(H) // 4, torch.arange(W) // 4
    blocks = ((hh[:, None] * 5 + ww[None, :]) % 3).double()                 # constant 4x4 blocks
    inputs = {"blocks": blocks[None, :, :, None].expand(N, H, W, C).contiguous(),
              "flat": torch.full((N, H, W, C), 1.5, dtype=torch.float64),
              "three": torch.tensor([-1.0, 0.0, 2.0], dtype=torch.float64)[
                  torch.randint(0, 3, (N, H, W, C))]}
    bad = []
    for name, x64 in inputs.items():
        for (k, s, p), ceil in itertools.product([(3, 2, 1), (2, 1, 0), (3, 1, 1), (2, 2, 0),
                                                  (3, 3, 0)], (False, True)):
            y, yr, dx, dxr, _ = _maxpool_both(x64.to(dtype).to(dev), k, s, p, ceil)
            if not torch.equal(y, yr) or not torch.equal(dx, dxr):
                bad.append((name, k, s, p, ceil))
    assert not bad, bad


_NAN = [(C, geo, dt) for C in (8, 64) for geo in ((3, 1, 1), (3, 2, 1), (2, 1, 0)) for dt in DTYPES]


@pytest.mark.parametrize("C,geo,dtype", _NAN, ids=_ids(_NAN))
def test_maxpool_nan(C, geo, dtype):
    """One NaN pixel per sample (channels of both argmax words), each covered by several windows:
    every window containing it outputs NaN and routes its gradient to that pixel alone, as torch's
    CPU float64 max-pool does."""
    k, s, p = geo
    N, H, W = 2, 9, 10
    at = [(3, 4), (5, 6)]
    chans = [1, 5] + ([C - 2] if C > 8 else [])
    x = torch.randn(N, H, W, C).to(dtype)
    for n, (h, w) in enumerate(at):
        x[n, h, w, chans] = float("nan")
    y, yr, dx, dxr, dy = _maxpool_both(x.to(dev), k, s, p, False)
    Ho, Wo = yr.shape[1:3]
    win = torch.zeros(N, Ho, Wo, C, dtype=torch.bool)        # windows (and channels) that see a NaN
    for n, (h, w) in enumerate(at):
        ho = [o for o in range(Ho) if o * s - p <= h <= o * s - p + k - 1]
        wo = [o for o in range(Wo) if o * s - p <= w <= o * s - p + k - 1]
        assert len(ho) * len(wo) >= 2
        for o in ho:
            win[n, o, wo[0]:wo[-1] + 1, chans] = True
    assert torch.equal(y.isnan(), win) and torch.equal(yr.isnan(), win)
    assert torch.equal(y.nan_to_num(0.0), yr.nan_to_num(0.0))
    assert not dxr.isnan().any() and torch.equal(dx, dxr)
    for n, (h, w) in enumerate(at):                            # the NaN pixel collects its windows
        assert torch.equal(dx[n, h, w, chans], (dy[n] * win[n]).sum((0, 1))[chans])
    # a gradient that lives on those windows only reaches no other pixel
    dy2 = dy * win
    _, _, dx2, dxr2, _ = _maxpool_both(x.to(dev), k, s, p, False, dy2)
    assert torch.equal(dx2, dxr2)
    for n, (h, w) in enumerate(at):
        dx2[n, h, w, chans] = 0.0
    assert not dx2.any()


_AG = [(k, s, p, C, dt) for k, s, p in ((2, 2, 0), (3, 1, 1), (5, 3, 0)) for C in (58, 64)
       for dt in DTYPES]


@pytest.mark.parametrize("k,s,p,C,dtype", _AG, ids=_ids(_AG))
def test_avgpool2d_geometry(k, s, p, C, dtype):
    """DenseNet's 2/2/0 and Inception's 3/1/1 and 5/3/0 pools on non-square inputs that the
    windows do not tile (rows / columns left over at the border, or windows cut by the padding)."""
    for H, W in ((17, 12), (9, 20)):
        assert (H - k) % s or (W - k) % s or p > 0
        _run_avgpool((2, H, W, C, k, s, p), dtype, "avg_geo")
