"""The Vision Transformer kernels (csrc/kernels/vit.hip) and the LayerNorm backward's stream
addend against the fp32 / fp64 contracts in mipipe.ops._ref."""
import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available
from mipipe.ops.determinism import deterministic

pytestmark = pytest.mark.gpu

dev = "cuda"
bf16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(1234)
    yield


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


# ------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("shape,P", [((3, 3, 32, 48), 16), ((2, 3, 64, 64), 32),
                                     ((2, 1, 32, 32), 16)])
@pytest.mark.parametrize("dtype", [torch.float32, bf16])
def test_patchify_bit_identical(shape, P, dtype):
    x = torch.randn(*shape, device=dev).to(dtype)
    got = native().patchify(x, P, bf16)
    want = _ref.patchify(x, P, torch.float32).to(bf16)
    B, C, H, W = shape
    assert got.shape == (B * (H // P) * (W // P), C * P * P) and got.dtype == bf16
    assert torch.equal(got, want)
    # fp32 rows (the reference precision): the values untouched
    assert torch.equal(native().patchify(x, P, torch.float32), _ref.patchify(x, P, torch.float32))


def test_patchify_full_tiles_and_tail():
    """More items than one block tile (1024) with a partial last tile: both loops run."""
    x = torch.randn(5, 3, 48, 80, device=dev)
    assert (x.numel() // 8) % 1024 != 0 and x.numel() // 8 > 4 * 1024
    assert torch.equal(native().patchify(x, 16, bf16), _ref.patchify(x, 16, bf16))


def test_patchify_bad_arguments_raise():
    x = torch.randn(2, 3, 32, 48, device=dev)
    with pytest.raises(RuntimeError, match="patches"):
        native().patchify(x[:, :, :30].contiguous(), 16, bf16)  # H % P
    with pytest.raises(RuntimeError, match="patches"):
        native().patchify(x[..., :40].contiguous(), 16, bf16)  # W % P
    with pytest.raises(RuntimeError, match="multiple of 8"):
        native().patchify(torch.randn(2, 3, 28, 28, device=dev), 14, bf16)  # P % 8
    with pytest.raises(RuntimeError, match="contiguous"):
        native().patchify(x.transpose(2, 3), 16, bf16)
    with pytest.raises(RuntimeError, match=r"\[B, C, H, W\]"):
        native().patchify(x[0], 16, bf16)
    with pytest.raises(RuntimeError, match="bfloat16 or float32"):
        native().patchify(x, 16, torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native().patchify(x.cpu(), 16, bf16)


# ----------------------------------------------------------------------- tokens_assemble
def _tokens(B, N, D, dtype=bf16):
    e = torch.randn(B * N, D, device=dev).to(dtype)
    cls = torch.randn(D, device=dev)
    pos = torch.randn((N + 1) * D, device=dev)
    return e, cls, pos


@pytest.mark.parametrize("D", [128, 768, 1032])
@pytest.mark.parametrize("dtype", [bf16, torch.float32])
def test_tokens_assemble_fwd_bit_identical(D, dtype):
    B, N = 3, 6
    e, cls, pos = _tokens(B, N, D, dtype)
    got = native().tokens_assemble_fwd(e, cls, pos)
    want = _ref.tokens_assemble_fwd(e, cls, pos)
    assert got.shape == (B * (N + 1), D) and got.dtype == dtype
    assert torch.equal(got, want)


def test_tokens_assemble_fwd_full_tiles_and_tail():
    B, N, D = 9, 12, 264  # 3861 items: three full block tiles and a partial one
    e, cls, pos = _tokens(B, N, D)
    assert torch.equal(native().tokens_assemble_fwd(e, cls, pos),
                       _ref.tokens_assemble_fwd(e, cls, pos))


@pytest.mark.parametrize("B,N,D", [(3, 6, 128), (3, 6, 768), (3, 6, 1032), (19, 4, 256)])
def test_tokens_assemble_bwd(B, N, D):
    """de is dh without the class rows, bit for bit; the batch sums against float64 at the
    tolerance test_layernorm_kernel_modes uses for fp32 column sums; accumulation into non-zero
    buffers; the same bits run to run and in deterministic mode.  B = 19: two unrolled groups
    of 8 batch rows and a remainder."""
    dh = torch.randn(B * (N + 1), D, device=dev).to(bf16)
    de, dpos, dcls = native().tokens_assemble_bwd(dh, B)
    g = dh.view(B, N + 1, D)
    assert de.shape == (B * N, D) and torch.equal(de, g[:, 1:].reshape(B * N, D))
    ref_pos = g.double().sum(0)
    assert dpos.dtype == torch.float32 and dpos.shape == ((N + 1) * D,)
    assert rel_err(dpos, ref_pos.reshape(-1)) < 1e-3
    assert rel_err(dcls, ref_pos[0]) < 1e-3
    # ascending-b fp32 sums: exactly the sequential sum
    seq = torch.zeros(N + 1, D, device=dev)
    for b in range(B):
        seq += g[b].float()
    assert torch.equal(dpos, seq.reshape(-1)) and torch.equal(dcls, seq[0])
    # accumulation into non-zero buffers (the flat gradient views)
    ap, ac = torch.randn((N + 1) * D, device=dev), torch.randn(D, device=dev)
    ap0, ac0 = ap.clone(), ac.clone()
    de2, none_p, none_c = native().tokens_assemble_bwd(dh, B, ap, ac)
    assert none_p is None and none_c is None and torch.equal(de2, de)
    assert torch.equal(ap, ap0 + dpos) and torch.equal(ac, ac0 + dcls)
    # run to run, and deterministic mode on / off
    again = native().tokens_assemble_bwd(dh, B)
    with deterministic(True):
        det = native().tokens_assemble_bwd(dh, B)
    for other in (again, det):
        for a, b in zip(other, (de, dpos, dcls)):
            assert torch.equal(a, b)


def test_tokens_assemble_bwd_fp32():
    B, N, D = 3, 6, 128
    dh = torch.randn(B * (N + 1), D, device=dev)
    de, dpos, dcls = native().tokens_assemble_bwd(dh, B)
    de_r, dpos_r, dcls_r = _ref.tokens_assemble_bwd(dh, B)
    assert torch.equal(de, de_r)
    assert rel_err(dpos, dpos_r) < 1e-3 and rel_err(dcls, dcls_r) < 1e-3


def test_tokens_assemble_bad_arguments_raise():
    e, cls, pos = _tokens(3, 6, 128)
    with pytest.raises(RuntimeError, match="must be"):
        native().tokens_assemble_fwd(e[:-1].contiguous(), cls, pos)  # not B*N rows
    with pytest.raises(RuntimeError, match="float32"):
        native().tokens_assemble_fwd(e, cls.to(bf16), pos)
    with pytest.raises(RuntimeError, match="whole rows"):
        native().tokens_assemble_fwd(e, cls, pos[:-1].contiguous())
    with pytest.raises(RuntimeError, match="multiple of 8"):
        native().tokens_assemble_fwd(torch.randn(18, 12, device=dev).to(bf16),
                                     torch.randn(12, device=dev), torch.randn(84, device=dev))
    dh = torch.randn(21, 128, device=dev).to(bf16)
    with pytest.raises(RuntimeError, match="batch"):
        native().tokens_assemble_bwd(dh, 4)
    with pytest.raises(RuntimeError, match="both accumulators"):
        native().tokens_assemble_bwd(dh, 3, torch.zeros(7 * 128, device=dev), None)
    with pytest.raises(RuntimeError, match="elements"):
        native().tokens_assemble_bwd(dh, 3, torch.zeros(6 * 128, device=dev),
                                     torch.zeros(128, device=dev))


# ---------------------------------------------------------------------- LayerNorm addend
@pytest.mark.parametrize("mode", [0, 4, 8, 16])
@pytest.mark.parametrize("H", [256, 512, 768, 1024, 1032])
@pytest.mark.parametrize("R", [37, 4100])
def test_layernorm_bwd_stream_addend(mode, H, R):
    """layernorm_bwd(..., dsum) on the (mode, H, R) grid of test_layernorm_kernel_modes: the exact
    widths 256 / 512 / 768 / 1024 at every wave count and the generic kernel (mode 0, H = 1032)."""
    old = native().get_layernorm_mode()
    native().set_layernorm_mode(mode)
    try:
        torch.manual_seed(H + R)
        x = torch.randn(R, H, device=dev).to(bf16)
        dy = torch.randn(R, H, device=dev).to(bf16)
        ds = torch.randn(R, H, device=dev).to(bf16)
        gma = torch.rand(H, device=dev) + 0.5
        bta = torch.randn(H, device=dev)
        _, mean, rstd, _ = native().layernorm_fwd(x, gma, bta, 1e-6)
        dx0, dg0, db0, _ = native().layernorm_bwd(dy, x, mean, rstd, gma)
        dacc = torch.zeros(H, device=dev)
        gacc, bacc = torch.zeros(H, device=dev), torch.zeros(H, device=dev)
        dx1, none_g, none_b, dxd = native().layernorm_bwd(dy, x, mean, rstd, gma, gacc, bacc,
                                                          dbias=dacc, dsum=ds)
        assert none_g is None and none_b is None and dxd is None
        dxr, _, _ = _ref.layernorm_bwd(dy.float(), x.float(), mean, rstd, gma, ds.float())
        assert rel_err(dx1, dxr) < 2e-2
        # one rounding, of the sum: every element within half a bf16 ulp (8 significant bits: at
        # most 2^-8 relative) of the
        # fp32 total, plus the fp32 evaluation-order noise of the two row sums (H <= 1032 terms:
        # ~sqrt(H) * 2^-24 of the row's magnitude, bounded here by 1e-5 of the largest total).
        # Rounding the LayerNorm part on its own first would miss by up to 2^-8 of THAT part,
        # hundreds of times this bound wherever the two parts cancel.
        tot = _ref.layernorm_bwd(dy.float(), x.float(), mean, rstd, gma)[0].float().double() \
            + ds.double()
        tol = tot.abs() * 2.0 ** -8 * 1.01 + 1e-5 * tot.abs().max()
        assert ((dx1.double() - tot).abs() <= tol).all()
        # the parameter gradients do not depend on the addend
        assert torch.equal(gacc, dg0) and torch.equal(bacc, db0)
        # the bias sum covers the stored total
        assert rel_err(dacc, dx1.float().sum(0)) < 1e-3
        # a zero addend changes nothing, without the bias sum as well
        dx2, dg2, db2, _ = native().layernorm_bwd(dy, x, mean, rstd, gma,
                                                  dsum=torch.zeros_like(ds))
        assert torch.equal(dx2, dx0) and torch.equal(dg2, dg0) and torch.equal(db2, db0)
    finally:
        native().set_layernorm_mode(old)


def test_layernorm_bwd_addend_refuses_dropout_and_bad_shapes():
    R, H = 16, 256
    x = torch.randn(R, H, device=dev).to(bf16)
    gma, bta = torch.ones(H, device=dev), torch.zeros(H, device=dev)
    _, mean, rstd, _ = native().layernorm_fwd(x, gma, bta, 1e-6)
    with pytest.raises(RuntimeError, match="dropout"):
        native().layernorm_bwd(x, x, mean, rstd, gma, None, None, 0.1, 7, None, None, x)
    with pytest.raises(ValueError, match="dropout"):
        K.layernorm_bwd(x, x, mean, rstd, gma, drop=(0.1, 7), dsum=x)
    with pytest.raises(RuntimeError, match="shape"):
        native().layernorm_bwd(x, x, mean, rstd, gma, dsum=x[:8].contiguous())
    with pytest.raises(RuntimeError, match="bfloat16"):
        native().layernorm_bwd(x, x, mean, rstd, gma, dsum=x.float())
