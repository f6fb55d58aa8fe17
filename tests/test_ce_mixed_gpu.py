"""Pair-target cross-entropy (Mixup / CutMix) on the MI355X: ``cross_entropy_mixed`` against
``_ref.cross_entropy_mixed_fwd_bwd`` and, at lambda = 1 and 0, bit for bit against the hard-label
``cross_entropy`` it shares its kernels with.

R = 131 is odd (the middle row pairs with itself); the vocabularies take the 8-wide vector path
(1000), the scalar path (1001, 10) and a padded vocabulary (1008 columns, 1003 classes).
Tolerances are those of test_kernels_gpu.py::test_cross_entropy_split_fwd_bwd."""
import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops.functional import cross_entropy, cross_entropy_mixed

pytestmark = pytest.mark.gpu

R = 131
GOUT = 0.37


@pytest.fixture(autouse=True)
def _native():
    from mipipe.ops._native import load_error, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _mix(lam):
    return torch.tensor([lam, 1, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")


def _run(fn, logits, *args, **kw):
    x = logits.clone().requires_grad_(True)
    loss = fn(x, *args, **kw)
    (loss * GOUT).backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("V,valid", [(1000, -1), (1001, -1), (10, -1), (1008, 1003)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_cross_entropy_mixed(V, valid, dtype):
    torch.manual_seed(1234 + V)
    logits = (torch.randn(R, V, device="cuda") * 3).to(dtype)
    labels = torch.randint(0, V if valid < 0 else valid, (R,), device="cuda")
    for eps in (0.0, 0.1):
        for lam in (1.0, 0.0, 0.3):
            mix = _mix(lam)
            loss, grad = _run(cross_entropy_mixed, logits, labels, mix, eps, valid_cols=valid)
            lr_, gr = _ref.cross_entropy_mixed_fwd_bwd(logits.float(), labels, mix, eps, valid)
            print(f"V={V} valid={valid} {dtype} eps={eps} lam={lam}: loss {loss.item():.7f} "
                  f"ref {lr_.item():.7f} grad rel_err {rel_err(grad, gr * GOUT):.3e}")
            assert loss.dtype == torch.float32 and grad.dtype == dtype
            assert abs(loss.item() - lr_.item()) <= 1e-4 * abs(lr_.item())
            assert rel_err(grad, gr * GOUT) < (1e-2 if dtype == torch.bfloat16 else 1e-5)
            if valid > 0:
                assert not grad[:, valid:].any()
            # two runs, identical bits (fixed-order loss sum, no float atomics)
            loss2, grad2 = _run(cross_entropy_mixed, logits, labels, mix, eps, valid_cols=valid)
            assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
            # lambda = 1 / 0: the hard-label kernels' bits for the own / the partner's labels
            if lam in (1.0, 0.0):
                hard = labels if lam == 1.0 else labels.flip(0)
                l0, g0 = _run(cross_entropy, logits, hard, eps, valid_cols=valid)
                assert torch.equal(loss, l0), (lam, eps, loss.item(), l0.item())
                assert torch.equal(grad, g0), (lam, eps)


def test_descriptor_rewritten_before_backward_is_an_error():
    """The backward reads lambda from the descriptor again, so a descriptor rewritten between a
    step's forward and its backward would give the gradient of another loss: the descriptor is
    saved for backward, and autograd's version check refuses that."""
    torch.manual_seed(7)
    logits = torch.randn(R, 1000, device="cuda")
    labels = torch.randint(0, 1000, (R,), device="cuda")
    mix = _mix(0.3)
    x = logits.clone().requires_grad_(True)
    loss = cross_entropy_mixed(x, labels, mix, 0.1)
    mix.copy_(_mix(1.0))
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_labels_outside_the_classes_read_nothing():
    """A label beyond the valid columns contributes a zero logit to the loss and no target."""
    torch.manual_seed(3)
    logits = torch.randn(5, 16, device="cuda")
    labels = torch.tensor([1, 2, 900, 4, 5], device="cuda")
    loss, grad = _run(cross_entropy_mixed, logits, labels, _mix(0.5), 0.0)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
