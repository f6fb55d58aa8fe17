"""The ConvNeXt kernels (csrc/kernels/dwconv7.hip, the 4-pixel patch path of vit.hip) against the
float64 evaluation of the contracts in mipipe.ops._ref, and the two existing kernels the family
leans on at new shapes: the GEMM at K = 48 and the dense 2x2 stride-2 convolution on odd maps.

Exact cases use small integers, so every product and partial sum is exactly representable and
``torch.equal`` applies whatever the summation order; random cases use a per-element bound from
the number of terms n and S = sum |terms| in float64: an fp32 accumulation (FMA or partial rows in
any order) is off by at most (n + 1) * 2^-24 * S to first order — doubled here — plus half an ulp
of the output format for the final rounding.
"""
import math

import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu

dev = "cuda"
bf16 = torch.bfloat16
DTYPES = [bf16, torch.float32]
ALL_DROPPED_SEED = 105  # found by tests/test_convnext_cpu.py::test_all_dropped_seed (N = 5, p = 0.5)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(4242)
    yield


def d(t):
    return None if t is None else t.detach().double().cpu()


def rel_err(a, b):
    a, b = d(a), d(b)
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def ints(lo, hi, *shape, dtype=torch.float32):
    return torch.randint(lo, hi + 1, shape, device=dev).to(dtype)


def half_ulp(dtype):
    return 2.0 ** -8 if dtype == bf16 else 2.0 ** -24  # unit roundoff: 8 / 24 significand bits


def within(got, ref, n_terms, s_abs, dtype):
    """|got - ref| <= 2 (n + 1) 2^-24 S + half_ulp(dtype) |ref| (+ the same for S's own size)."""
    bound = 2.0 * (n_terms + 1) * 2.0 ** -24 * s_abs + half_ulp(dtype) * (ref.abs() + 2.0 ** -24 * s_abs)
    err = (d(got) - ref).abs()
    return bool((err <= bound + 1e-300).all()), float((err - bound).max())


def _tiles():
    C = native()
    return C.DW7_TILE_H, C.DW7_TILE_W


def _maps():
    th, tw = _tiles()
    return [(1, 1), (2, 3), (6, 6), (7, 7), (8, 8), (9, 23), (14, 14), (th + 1, tw + 1),
            (th - 1, tw - 1)]


MAP_IDS = list(range(9))
CHANNELS = [8, 40, 96, 2048]
BATCHES = [1, 3]


def _wgrad_rows(N, H, W, C, dtype):
    """csrc/kernels/convnext.hpp dw7_wgrad_rows from the exported constants."""
    c = native()
    cb = c.DW7_CHAN_BLOCK if dtype == bf16 else c.DW7_CHAN_BLOCK_F32
    ncb = -(-C // cb)
    p = min(max(c.DW7_WGRAD_BLOCKS // ncb, c.DW7_WGRAD_MIN_ROWS), c.DW7_WGRAD_MAX_ROWS)
    return min(p, N * -(-H // c.DW7_TILE_H) * -(-W // c.DW7_TILE_W))


# ------------------------------------------------------------------------------ dwconv7: exact
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("mi", MAP_IDS)
def test_dwconv7_exact(mi, dtype):
    """Integer x, dy in [-2, 2], w in {-1, 0, 1}, small integer bias: |sum| <= 49 * 2 + 4 < 256, so
    bf16 holds every output and the fp32 weight-grad sums stay far below 2^24."""
    H, W = _maps()[mi]
    for C in CHANNELS:
        for N in BATCHES:
            x = ints(-2, 2, N, H, W, C, dtype=dtype)
            dy = ints(-2, 2, N, H, W, C, dtype=dtype)
            add = ints(-2, 2, N, H, W, C, dtype=dtype)
            w = ints(-1, 1, C, 7, 7, 1, dtype=dtype)
            b = ints(-4, 4, C)
            tag = (H, W, C, N)
            y = K.dwconv7_fwd(x, w, b)
            assert y.dtype == dtype and torch.equal(d(y), _ref.dwconv7_fwd(d(x), d(w), d(b))), tag
            assert torch.equal(d(K.dwconv7_fwd(x, w)), _ref.dwconv7_fwd(d(x), d(w))), tag
            assert torch.equal(d(K.dwconv7_dgrad(dy, w)), _ref.dwconv7_dgrad(d(dy), d(w))), tag
            assert torch.equal(d(K.dwconv7_dgrad(dy, w, add)),
                               _ref.dwconv7_dgrad(d(dy), d(w), d(add))), tag
            dwr, dbr = _ref.dwconv7_wgrad(d(dy), d(x))
            dw, db = K.dwconv7_wgrad(dy, x)
            assert dw.shape == (C, 1, 7, 7) and dw.dtype == torch.float32
            assert torch.equal(d(dw), dwr) and torch.equal(d(db), dbr), tag
            # the contract is +=: pre-filled accumulators
            aw, ab = ints(-8, 8, C, 1, 7, 7), ints(-8, 8, C)
            aw0, ab0 = aw.clone(), ab.clone()
            r = K.dwconv7_wgrad(dy, x, aw.reshape(-1), ab)
            assert r[0] is None and r[1] is None
            assert torch.equal(d(aw), d(aw0) + dwr) and torch.equal(d(ab), d(ab0) + dbr), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_dwconv7_wgrad_many_rows(dtype):
    """More tiles than partial rows (a block walks several tiles) and more partial rows than the
    fixed-order finish takes in one level (4 * DET_CHUNK_ROWS): exact, and the same bits twice."""
    c = native()
    N, a = 3, 14
    b = (c.DW7_WGRAD_MAX_ROWS + 1 + N * a - 1) // (N * a)
    H, W, C = a * c.DW7_TILE_H - 3, b * c.DW7_TILE_W - 5, 8
    P = _wgrad_rows(N, H, W, C, dtype)
    assert N * a * b > P > 4 * c.DET_CHUNK_ROWS
    x = ints(-2, 2, N, H, W, C, dtype=dtype)
    dy = ints(-2, 2, N, H, W, C, dtype=dtype)
    dwr, dbr = _ref.dwconv7_wgrad(d(dy), d(x))
    dw, db = K.dwconv7_wgrad(dy, x)
    assert torch.equal(d(dw), dwr) and torch.equal(d(db), dbr)
    dw2, db2 = K.dwconv7_wgrad(dy, x)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_dwconv7_past_the_grid_cap(dtype):
    """More tiles than DW7_MAX_BLOCKS spatial blocks: some blocks of the forward / data-grad kernel
    walk a second tile (halo refilled behind the barrier, accumulators started again from the
    bias), others do not.  Exact integer case, with the bias and with the data-grad's addend."""
    c = native()
    N, a = 3, 38
    b = (c.DW7_MAX_BLOCKS + 1 + N * a - 1) // (N * a)
    H, W, C = a * c.DW7_TILE_H - 3, b * c.DW7_TILE_W - 5, 8
    tiles = N * -(-H // c.DW7_TILE_H) * -(-W // c.DW7_TILE_W)
    assert c.DW7_MAX_BLOCKS < tiles < 2 * c.DW7_MAX_BLOCKS
    x = ints(-2, 2, N, H, W, C, dtype=dtype)
    add = ints(-2, 2, N, H, W, C, dtype=dtype)
    w = ints(-1, 1, C, 7, 7, 1, dtype=dtype)
    bias = ints(-4, 4, C)
    assert torch.equal(d(K.dwconv7_fwd(x, w, bias)), _ref.dwconv7_fwd(d(x), d(w), d(bias)))
    assert torch.equal(d(K.dwconv7_dgrad(x, w, add)), _ref.dwconv7_dgrad(d(x), d(w), d(add)))
    assert torch.equal(d(K.dwconv7_dgrad(x, w)), _ref.dwconv7_dgrad(d(x), d(w)))


# ----------------------------------------------------------------------------- dwconv7: random
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(3, 9, 23, 40), (2, 14, 14, 96), (1, 7, 7, 2048),
                                   (2, 30, 37, 8)])
def test_dwconv7_random_within_summation_bound(shape, dtype):
    N, H, W, C = shape
    x = torch.randn(N, H, W, C, device=dev).to(dtype)
    dy = torch.randn(N, H, W, C, device=dev).to(dtype)
    add = torch.randn(N, H, W, C, device=dev).to(dtype)
    w = (torch.randn(C, 7, 7, 1, device=dev) / 7).to(dtype)
    b = torch.randn(C, device=dev)
    ref = _ref.dwconv7_fwd(d(x), d(w), d(b))
    s = _ref.dwconv7_fwd(d(x).abs(), d(w).abs(), d(b).abs())
    ok, over = within(K.dwconv7_fwd(x, w, b), ref, 50, s, dtype)
    assert ok, over
    ref = _ref.dwconv7_dgrad(d(dy), d(w), d(add))
    s = _ref.dwconv7_dgrad(d(dy).abs(), d(w).abs(), d(add).abs())
    ok, over = within(K.dwconv7_dgrad(dy, w, add), ref, 50, s, dtype)
    assert ok, over
    dwr, dbr = _ref.dwconv7_wgrad(d(dy), d(x))
    sw, sb = _ref.dwconv7_wgrad(d(dy).abs(), d(x).abs())
    dw, db = K.dwconv7_wgrad(dy, x)
    n = N * H * W + 1024  # the pixels plus the partial rows' own sums
    ok, over = within(dw, dwr, n, sw, torch.float32)
    assert ok, over
    ok, over = within(db, dbr, n, sb, torch.float32)
    assert ok, over
    # reproducible: no float atomics in any mode
    dw2, db2 = K.dwconv7_wgrad(dy, x)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_dwconv7_bad_arguments_raise():
    x = torch.randn(2, 8, 8, 16, device=dev).to(bf16)
    w = torch.randn(16, 7, 7, 1, device=dev).to(bf16)
    n = native()
    with pytest.raises(RuntimeError, match="C % 8"):
        n.dwconv7_fwd(torch.zeros(1, 4, 4, 12, device=dev, dtype=bf16),
                      torch.zeros(12, 7, 7, 1, device=dev, dtype=bf16))
    with pytest.raises(RuntimeError, match="C <= 2048"):
        n.dwconv7_fwd(torch.zeros(1, 2, 2, 2056, device=dev, dtype=bf16),
                      torch.zeros(2056, 7, 7, 1, device=dev, dtype=bf16))
    with pytest.raises(RuntimeError, match="w must be"):
        n.dwconv7_fwd(x, w.reshape(16, 1, 7, 7))
    with pytest.raises(RuntimeError, match="w must be"):
        n.dwconv7_dgrad(x, torch.zeros(16, 3, 3, 1, device=dev, dtype=bf16))
    with pytest.raises(RuntimeError, match="contiguous"):
        n.dwconv7_fwd(x.transpose(1, 2), w)
    with pytest.raises(RuntimeError, match="bfloat16 or float32"):
        n.dwconv7_fwd(x.half(), w.half())
    with pytest.raises(RuntimeError, match="like the other operands"):
        n.dwconv7_fwd(x, w.float())
    with pytest.raises(RuntimeError, match="GPU tensor"):
        n.dwconv7_fwd(x.cpu(), w.cpu())
    with pytest.raises(RuntimeError, match="empty"):
        n.dwconv7_fwd(x[:0], w)
    with pytest.raises(RuntimeError, match="shape"):
        n.dwconv7_dgrad(x, w, x[:1])
    with pytest.raises(RuntimeError, match="shape"):
        n.dwconv7_wgrad(x[:1], x)
    with pytest.raises(RuntimeError, match="elements"):
        n.dwconv7_wgrad(x, x, torch.zeros(16 * 48, device=dev))
    with pytest.raises(RuntimeError, match="elements"):
        n.dwconv7_fwd(x, w, torch.zeros(8, device=dev))


# ------------------------------------------------------------------------------ scale_residual
def _sr_inputs(N, hw, C, dtype):
    f = torch.randn(N, hw, C, device=dev).to(dtype)
    res = torch.randn(N, hw, C, device=dev).to(dtype)
    dout = torch.randn(N, hw, C, device=dev).to(dtype)
    gamma = torch.randn(C, device=dev)
    return f, res, dout, gamma


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("p", [0.0, 0.3, 0.5])
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("C", [8, 96, 1536])
def test_scale_residual_bit_identical(C, N, p, dtype):
    """Forward and df equal the three-rounding contract bit for bit (rows 63 per sample: neither
    the forward's tile nor the backward's SR_BLOCK_ROWS divides them); the column sums lie within
    the summation bound, repeat bit for bit and respect pre-filled accumulators."""
    hw, seed = 63, 1234 + N
    assert (N * hw) % native().SR_BLOCK_ROWS
    f, res, dout, gamma = _sr_inputs(N, hw, C, dtype)
    out = K.scale_residual_fwd(f, res, gamma, hw, p, seed)
    assert out.dtype == dtype and torch.equal(out, _ref.scale_residual_fwd(f, res, gamma, hw, p, seed))
    df, dg, db = K.scale_residual_bwd(dout, f, gamma, hw, p, seed, want_bias=True)
    dfr, _, _ = _ref.scale_residual_bwd(dout, f, gamma, hw, p, seed)
    assert torch.equal(df, dfr)
    if p > 0 and N > 1:
        keep = _ref.drop_path_keep(N, p, seed, dev)
        assert torch.equal((df.reshape(N, -1) != 0).any(1), keep)
    # float64 references of the sums, over the values the kernel sums (s_n in fp32, df as stored)
    s = _ref._path_scale(f, hw, p, seed).double().cpu()
    terms = d(dout).reshape(-1, C) * d(f).reshape(-1, C) * s
    ok, over = within(dg, terms.sum(0), N * hw + 64, terms.abs().sum(0), torch.float32)
    assert ok, over
    ok, over = within(db, d(df).reshape(-1, C).sum(0), N * hw + 64,
                      d(df).reshape(-1, C).abs().sum(0), torch.float32)
    assert ok, over
    df2, dg2, db2 = K.scale_residual_bwd(dout, f, gamma, hw, p, seed, want_bias=True)
    assert torch.equal(df, df2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    _, dg3, db3 = K.scale_residual_bwd(dout, f, gamma, hw, p, seed)
    assert db3 is None and torch.equal(dg3, dg)  # the bias sum is optional


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,N,hw", [(8, 5, 63), (96, 5, 200), (1536, 2, 77)])
def test_scale_residual_sums_exact(C, N, hw, dtype):
    """gamma powers of two, p = 0.5 (s_n in {0, 2}), integer dout and f: every term and every sum
    is an exact integer, so the column sums equal float64 whatever the order; ``+=`` holds."""
    p, seed = 0.5, 99
    f = ints(-3, 3, N, hw, C, dtype=dtype)
    dout = ints(-3, 3, N, hw, C, dtype=dtype)
    gamma = torch.pow(2.0, torch.randint(-2, 3, (C,), device=dev).float())
    df, dg, db = K.scale_residual_bwd(dout, f, gamma, hw, p, seed, want_bias=True)
    dfr, dgr, dbr = _ref.scale_residual_bwd(d(dout), d(f), d(gamma), hw, p, seed)
    assert torch.equal(d(df), dfr) and torch.equal(d(dg), dgr) and torch.equal(d(db), dbr)
    ag, ab = ints(-8, 8, C), ints(-8, 8, C)
    ag0, ab0 = ag.clone(), ab.clone()
    _, rg, rb = K.scale_residual_bwd(dout, f, gamma, hw, p, seed, ag, ab)
    assert rg is None and rb is None
    assert torch.equal(d(ag), d(ag0) + dgr) and torch.equal(d(ab), d(ab0) + dbr)


def _dd(t):
    """float64 on the device: the references of the cases past the grid caps (tens of MB)"""
    return t.detach().double()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,N", [(1536, 3), (96, 5)])
def test_scale_residual_bwd_past_the_grid_cap(C, N, dtype):
    """More rows than SR_MAX_BLOCKS / ncc blocks take in one pass of SR_BLOCK_ROWS: a block's
    register accumulators carry over two to three passes, the last one partial.  The power-of-two
    construction (|sum| <= 18 R < 2^24), so ``torch.equal`` against float64 holds."""
    c = native()
    ncc = -(-C // 64)
    per_pass = max(c.SR_MAX_BLOCKS // ncc, 1) * c.SR_BLOCK_ROWS
    hw = (2 * per_pass + per_pass // 3) // N + 1
    R = N * hw
    assert 2 * per_pass < R < 3 * per_pass and R % c.SR_BLOCK_ROWS and 18 * R < 2 ** 24
    p, seed = 0.5, 99
    f = ints(-3, 3, N, hw, C, dtype=dtype)
    dout = ints(-3, 3, N, hw, C, dtype=dtype)
    gamma = torch.pow(2.0, torch.randint(-2, 3, (C,), device=dev).float())
    ag, ab = ints(-8, 8, C), ints(-8, 8, C)
    ag0, ab0 = ag.clone(), ab.clone()
    df, rg, rb = K.scale_residual_bwd(dout, f, gamma, hw, p, seed, ag, ab)
    dfr, dgr, dbr = _ref.scale_residual_bwd(_dd(dout), _dd(f), _dd(gamma), hw, p, seed)
    assert rg is None and rb is None and 0 < int(_ref.drop_path_keep(N, p, seed).sum()) < N
    assert torch.equal(_dd(df), dfr)
    assert torch.equal(_dd(ag), _dd(ag0) + dgr) and torch.equal(_dd(ab), _dd(ab0) + dbr)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_scale_residual_fwd_past_the_grid_cap(dtype):
    """More items than SR_FWD_MAX_BLOCKS blocks stream in one tile each: every block takes a
    second tile, some a third, the last tile partial; bit-identical to the contract.  The backward
    on the same tensors (three passes at C = 96) gives the contract's df bit for bit."""
    c = native()
    C, N, p, seed = 96, 5, 0.3, 4323  # keeps samples 1, 2, 3
    one_pass = c.SR_FWD_MAX_BLOCKS * c.SR_FWD_TILE  # 8-channel items
    hw = (2 * one_pass + one_pass // 4) // (N * (C // 8)) + 1
    items = N * hw * (C // 8)
    assert 2 * one_pass < items < 3 * one_pass and items % c.SR_FWD_TILE
    f, res, dout, gamma = _sr_inputs(N, hw, C, dtype)
    assert 0 < int(_ref.drop_path_keep(N, p, seed).sum()) < N
    assert torch.equal(K.scale_residual_fwd(f, res, gamma, hw, p, seed),
                       _ref.scale_residual_fwd(f, res, gamma, hw, p, seed))
    assert torch.equal(K.scale_residual_fwd(f, res, gamma, hw, 0.0, 0),
                       _ref.scale_residual_fwd(f, res, gamma, hw, 0.0, 0))
    df, _, _ = K.scale_residual_bwd(dout, f, gamma, hw, p, seed)
    assert torch.equal(df, _ref.scale_residual_bwd(dout, f, gamma, hw, p, seed)[0])


def test_scale_residual_eval_and_dev_seed():
    N, hw, C, p = 5, 63, 96, 0.5
    f, res, dout, gamma = _sr_inputs(N, hw, C, bf16)
    g3 = gamma.reshape(C, 1, 1)
    # evaluation (and p = 0) drops nothing: s_n = 1
    ev = MF.scale_residual(f, res, g3, p, 7, training=False)
    assert torch.equal(ev, _ref.scale_residual_fwd(f, res, gamma, hw, 0.0, 0))
    assert torch.equal(ev, MF.scale_residual(f, res, g3, 0.0, 7, training=True))
    # a device-counter seed draws the masks of its host-folded seed, forward and backward
    ctr = torch.full((1,), 5, dtype=torch.int32, device=dev)
    dseed, hseed = K.DevSeed(77, ctr), _ref.fold_dev_seed(77, 5)
    assert torch.equal(K.scale_residual_fwd(f, res, gamma, hw, p, dseed),
                       K.scale_residual_fwd(f, res, gamma, hw, p, hseed))
    a = K.scale_residual_bwd(dout, f, gamma, hw, p, dseed, want_bias=True)
    b = K.scale_residual_bwd(dout, f, gamma, hw, p, hseed, want_bias=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(K.drop_path_keep(N, p, dseed, dev), _ref.drop_path_keep(N, p, hseed, dev))
    ctr.add_(1)  # the next step: another mask from the same call
    assert not torch.equal(K.drop_path_keep(64, p, dseed, dev), _ref.drop_path_keep(64, p, hseed, dev))
    assert torch.equal(K.scale_residual_fwd(f, res, gamma, hw, p, dseed),
                       K.scale_residual_fwd(f, res, gamma, hw, p, _ref.fold_dev_seed(77, 6)))


def test_scale_residual_all_dropped_batch():
    """Every sample dropped: out = res, df = 0 and the sums add exact zeros — every kernel still
    runs and every accumulator is still written."""
    N, hw, C, p = 5, 63, 96, 0.5
    assert not bool(_ref.drop_path_keep(N, p, ALL_DROPPED_SEED).any())
    f, res, dout, gamma = _sr_inputs(N, hw, C, bf16)
    assert torch.equal(K.scale_residual_fwd(f, res, gamma, hw, p, ALL_DROPPED_SEED), res)
    ag, ab = ints(-8, 8, C), ints(-8, 8, C)
    ag0, ab0 = ag.clone(), ab.clone()
    df, _, _ = K.scale_residual_bwd(dout, f, gamma, hw, p, ALL_DROPPED_SEED, ag, ab)
    assert not bool(df.any()) and torch.equal(ag, ag0) and torch.equal(ab, ab0)


def test_scale_residual_bad_arguments_raise():
    n = native()
    f = torch.randn(2, 6, 16, device=dev).to(bf16)
    g = torch.ones(16, device=dev)
    with pytest.raises(RuntimeError, match="C % 8"):
        n.scale_residual_fwd(f[..., :12].contiguous(), f[..., :12].contiguous(), g[:12], 6)
    with pytest.raises(RuntimeError, match="whole samples"):
        n.scale_residual_fwd(f, f, g, 5)
    with pytest.raises(RuntimeError, match="shape"):
        n.scale_residual_fwd(f, f[:1], g, 6)
    with pytest.raises(RuntimeError, match="elements"):
        n.scale_residual_fwd(f, f, g[:8], 6)
    with pytest.raises(RuntimeError, match="probability"):
        n.scale_residual_fwd(f, f, g, 6, 1.0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        n.scale_residual_fwd(f.cpu(), f.cpu(), g.cpu(), 6)
    with pytest.raises(RuntimeError, match="empty"):
        n.scale_residual_fwd(f[:0], f[:0], g, 6)


# ------------------------------------------------------------------------------ patchify, P = 4
@pytest.mark.parametrize("dtypes", [(torch.float32, bf16), (bf16, bf16),
                                    (torch.float32, torch.float32)], ids=["f32-bf16", "bf16", "f32"])
@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (5, 3, 64, 72), (3, 3, 36, 44), (1, 1, 4, 4)])
def test_patchify4_bit_identical(shape, dtypes):
    """4-pixel patches: below one tile of the streaming kernel, several full tiles with a guarded
    tail, an odd patch grid, a single patch."""
    ti, to = dtypes
    x = torch.randn(*shape, device=dev).to(ti)
    got = native().patchify(x, 4, to)
    assert got.dtype == to and got.shape == (shape[0] * shape[2] * shape[3] // 16, shape[1] * 16)
    assert torch.equal(got, _ref.patchify(x, 4, to))


@pytest.mark.parametrize("N", [40, 96])
def test_stem_gemm_k48(N):
    """The stem's GEMM: K = 3 * 4 * 4 = 48, below the kernels' 64-deep k-step."""
    M, Kd = 320, 48
    a = torch.randn(M, Kd, device=dev).to(bf16)
    b = (torch.randn(N, Kd, device=dev) / math.sqrt(Kd)).to(bf16)
    bias = torch.randn(N, device=dev)
    ref = _ref.gemm(d(a), d(b), False, True, d(bias), "none", torch.float64)
    out = native().gemm(a, b, False, True, bias, "none", bf16, None, 0.0)
    assert rel_err(out, ref) < 1e-2
    out32 = native().gemm(a, b, False, True, bias, "none", torch.float32, None, 0.0)
    assert rel_err(out32, ref) < 2e-3
    # the weight-grad GEMM of the same layer (the image takes no gradient: no data-grad)
    dy = torch.randn(M, N, device=dev).to(bf16)
    dwr = _ref.gemm(d(dy), d(a), True, False, None, "none", torch.float64)
    assert rel_err(native().gemm(dy, a, True, False, None, "none", torch.float32, None, 0.0), dwr) < 2e-3


# ----------------------------------------------------------- the 2x2 stride-2 downsample conv
@pytest.mark.parametrize("hw", [4, 5])
def test_downsample_conv_fp32(hw):
    """40 -> 80 channels, 2x2 / 2, on an even and an odd map (5 -> 2: the last row and column are
    read by no window and get a zero gradient), at test_fp32_gpu.py's tolerance."""
    N, Ci, Co, TOL = 3, 40, 80, 1e-4
    ho = (hw - 2) // 2 + 1
    x = torch.randn(N, hw, hw, Ci, device=dev)
    w = torch.randn(Co, 2, 2, Ci, device=dev) / math.sqrt(4 * Ci)
    dy = torch.randn(N, ho, ho, Co, device=dev)
    y, _, _ = native().conv_fwd(x, w, 2, 0, None)
    assert y.shape == (N, ho, ho, Co)
    assert rel_err(y, _ref.conv_fwd(d(x), d(w), 2, 0)[0]) < TOL
    dx = native().conv_dgrad(dy, w, [N, hw, hw, Ci], 2, 0)
    assert rel_err(dx, _ref.conv_dgrad(d(dy), d(w), (N, hw, hw, Ci), 2, 0)) < TOL
    dw = native().conv_wgrad(dy, x, 2, 2, 2, 0)
    assert rel_err(dw, _ref.conv_wgrad(d(dy), d(x), 2, 2, 2, 0)) < TOL


@pytest.mark.parametrize("hw", [4, 5])
def test_downsample_conv_bf16(hw):
    """The same layer in the precision the model runs it, at test_kernels_gpu.py's tolerances."""
    N, Ci, Co = 3, 40, 80
    ho = (hw - 2) // 2 + 1
    x = torch.randn(N, hw, hw, Ci, device=dev).to(bf16)
    w = (torch.randn(Co, 2, 2, Ci, device=dev) / math.sqrt(4 * Ci)).to(bf16)
    dy = torch.randn(N, ho, ho, Co, device=dev).to(bf16)
    bias = torch.randn(Co, device=dev)
    y, _, _ = native().conv_fwd(x, w, 2, 0, None, None, None, bias, False)
    yr = _ref.conv_fwd(d(x), d(w), 2, 0)[0] + d(bias)
    assert rel_err(y, yr) < 1e-2
    dx = native().conv_dgrad(dy, w, [N, hw, hw, Ci], 2, 0)
    assert rel_err(dx, _ref.conv_dgrad(d(dy), d(w), (N, hw, hw, Ci), 2, 0)) < 1e-2
    dw = native().conv_wgrad(dy, x, 2, 2, 2, 0)
    assert rel_err(dw, _ref.conv_wgrad(d(dy), d(x), 2, 2, 2, 0)) < 5e-3
