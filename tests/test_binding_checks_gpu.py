"""The argument checks the Python entries share (csrc/bind/common.hpp): ``ce_args`` for the five
cross-entropy entries, ``top1_correct`` and ``eval_stats``; ``check_records`` for
``record_decode``, ``record_decode_rrc`` and ``record_augment``.

Every wrong call must raise ``RuntimeError`` with the shared checker's own message, on the host,
before anything is launched (labels on another GPU, the one fault that three entries newly
refuse, needs two devices and has no case here); one valid
call per family, at the same shapes, must return what ``_ref`` returns, so the shared checkers
reject nothing valid.  Shapes: logits [4, 16] bf16, records [2, 1 + 3*4*4] uint8.

Tolerances of the valid cross-entropy calls (the integer results and the record kernels, whose
contract is bit-identity with ``_ref``, are compared exactly):

* loss: the kernels use the hardware exp / log (about 1 ulp of fp32 each; the multiply by log2(e)
  inside exp turns the rounding of an argument of up to ~10 into a relative error of up to
  ~6e-7), so a row's log-sum-exp of a few units is off by up to ~2e-6 absolute, and so is the mean
  over the rows; ``_ref`` adds its own fp32 rounding.  Bound: 1e-5 absolute.
* gradient: bf16, computed in fp32 on both sides and rounded once, so the two may land on
  neighbouring bf16 values where the fp32 results straddle a rounding boundary: at most one bf16
  ulp, which is at most 2^-7 relative to the value.  Where the softmax nearly cancels its target
  the fp32 error of the softmax itself shows instead (2e-6 of a probability of at most 1, over
  R = 4 rows): 5e-7 absolute on top.
"""
import pytest
import torch

from mipipe.ops import _ref

pytestmark = pytest.mark.gpu

R, V = 4, 16
C, H, W, LB = 3, 4, 4, 1
N = 2
Q24 = float(1 << 24)


@pytest.fixture(scope="module")
def nat():
    from mipipe.ops._native import load_error, native, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"
    return native()


def _ce_inputs():
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(R, V, generator=g) * 3).to(torch.bfloat16).cuda()
    labels = torch.randint(0, V, (R,), generator=g).cuda()
    return logits, labels


def _mix(lam=0.3):
    return torch.tensor([lam, 1, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")


def _work():
    return torch.zeros(4 + 2 * R, dtype=torch.int32, device="cuda")


def _gout(n=1):
    return torch.ones(n, dtype=torch.float32, device="cuda")


def _counters():
    return torch.zeros(8, dtype=torch.int64, device="cuda")


# name -> call(_C, logits, labels, work=..., gout=...)
CE_ENTRIES = {
    "cross_entropy_fwd": lambda c, lg, lb, **k: c.cross_entropy_fwd(lg, lb),
    "cross_entropy_bwd": lambda c, lg, lb, work=None, gout=None: c.cross_entropy_bwd(
        lg, lb, _work() if work is None else work, _gout() if gout is None else gout),
    "cross_entropy_fwd_bwd": lambda c, lg, lb, **k: c.cross_entropy_fwd_bwd(lg, lb, 0.0, -100),
    "cross_entropy_mixed_fwd": lambda c, lg, lb, **k: c.cross_entropy_mixed_fwd(lg, lb, _mix()),
    "cross_entropy_mixed_bwd": lambda c, lg, lb, work=None, gout=None: c.cross_entropy_mixed_bwd(
        lg, lb, _mix(), _work() if work is None else work, _gout() if gout is None else gout),
    "top1_correct": lambda c, lg, lb, **k: c.top1_correct(lg, lb),
    "eval_stats": lambda c, lg, lb, **k: c.eval_stats(lg, lb, _counters()),
}


def _bad_ce(case):
    logits, labels = _ce_inputs()
    if case == "labels_int32":
        labels = labels.to(torch.int32)
    elif case == "labels_len3":
        labels = labels[:3].contiguous()
    elif case == "labels_cpu":
        labels = labels.cpu()
    elif case == "logits_noncontig":
        logits = logits.t().contiguous().t()
        assert logits.shape == (R, V) and not logits.is_contiguous()
    return logits, labels


# what ce_args itself says of each fault (torch's own data_ptr<T>() check says none of these)
CE_MESSAGE = {"labels_int32": "labels must be int64", "labels_len3": "shape mismatch",
              "labels_cpu": "labels must be a GPU tensor",
              "logits_noncontig": "logits must be contiguous"}


@pytest.mark.parametrize("case", list(CE_MESSAGE))
@pytest.mark.parametrize("entry", list(CE_ENTRIES))
def test_ce_family_rejects(nat, entry, case):
    logits, labels = _bad_ce(case)
    with pytest.raises(RuntimeError, match=CE_MESSAGE[case]):
        CE_ENTRIES[entry](nat, logits, labels)


@pytest.mark.parametrize("case", ["work_len", "gout_two"])
@pytest.mark.parametrize("entry", ["cross_entropy_bwd", "cross_entropy_mixed_bwd"])
def test_ce_backward_rejects(nat, entry, case):
    logits, labels = _ce_inputs()
    kw = {"work": torch.zeros(4 + 2 * R + 1, dtype=torch.int32, device="cuda")} \
        if case == "work_len" else {"gout": _gout(2)}
    msg = "CE work buffer mismatch" if case == "work_len" else "gout must be one value"
    with pytest.raises(RuntimeError, match=msg):
        CE_ENTRIES[entry](nat, logits, labels, **kw)


def _close_ce(loss, grad, ref_loss, ref_grad):
    assert loss.dtype == torch.float32 and grad.dtype == torch.bfloat16
    dl = abs(loss.item() - ref_loss.item())
    d = (grad.float() - ref_grad.float()).abs()
    bound = ref_grad.float().abs() * 2.0 ** -7 + 5e-7
    print(f"loss {loss.item():.7f} ref {ref_loss.item():.7f} diff {dl:.2e}; "
          f"grad worst diff / bound {(d / bound).max().item():.3f}")
    assert dl <= 1e-5
    assert bool((d <= bound).all())


def test_ce_family_accepts(nat):
    logits, labels = _ce_inputs()
    ref_loss, ref_grad = _ref.cross_entropy_fwd_bwd(logits, labels)
    loss, work = nat.cross_entropy_fwd(logits, labels)
    _close_ce(loss, nat.cross_entropy_bwd(logits, labels, work, _gout()), ref_loss, ref_grad)
    _close_ce(*nat.cross_entropy_fwd_bwd(logits, labels, 0.0, -100), ref_loss, ref_grad)
    mix = _mix()
    ref_loss, ref_grad = _ref.cross_entropy_mixed_fwd_bwd(logits, labels, mix)
    loss, work = nat.cross_entropy_mixed_fwd(logits, labels, mix)
    _close_ce(loss, nat.cross_entropy_mixed_bwd(logits, labels, mix, work, _gout()), ref_loss,
              ref_grad)


def test_metrics_accept(nat):
    logits, labels = _ce_inputs()
    labels = logits.float().argmax(1).where(torch.arange(R, device="cuda") % 2 == 0, labels)
    want = int((logits.float().argmax(1) == labels).sum())
    assert nat.top1_correct(logits, labels).tolist() == [want] and want >= 2
    got, ref = _counters(), _counters()
    nat.eval_stats(logits, labels, got, None, None, 5, -100, -1)
    _ref.eval_stats(logits, labels, ref, None, None, 5, -100, -1)
    print("counters", got.tolist(), "ref", ref.tolist())
    assert got[:5].tolist() == ref[:5].tolist() and got[6:].tolist() == [0, 0]
    assert got[:2].tolist() == [R, want]
    # the Q24 loss sum: R rows, each within the loss bound of the module docstring
    assert abs(got[5].item() - ref[5].item()) / Q24 <= R * 1e-5


# ------------------------------------------------------------------------------------ records
def _records():
    g = torch.Generator().manual_seed(5)
    rec = torch.randint(0, 256, (N, LB + C * H * W), generator=g, dtype=torch.uint8).cuda()
    idx = torch.tensor([7, 123456789], dtype=torch.int64, device="cuda")
    affine = torch.tensor([[1 / 255, 2 / 255, 0.5 / 255], [-0.5, 0.25, 0.0]], device="cuda")
    return rec, idx, affine


REC_ENTRIES = {
    "record_decode": lambda c, rec, idx, aff, lb: c.record_decode(
        rec, idx, aff, C, H, W, 3, 2, 1, True, True, lb, torch.float32),
    "record_decode_rrc": lambda c, rec, idx, aff, lb: c.record_decode_rrc(
        rec, idx, aff, C, H, W, 4, 4, 3, 2, True, True, lb, torch.float32),
    "record_augment": lambda c, rec, idx, aff, lb: c.record_augment(rec, idx, C, H, W, 3, 2, lb),
}


# what check_records / check_sample_idx themselves say of each fault
REC_MESSAGE = {"rec_int8": "rec must be uint8", "idx_int32": "idx must be int64",
               "idx_len1": r"idx must be \[n\]", "label_bytes_0": "label_bytes must be in",
               "label_bytes_9": "label_bytes must be in", "rec_wide": r"rec must be \[n, "}


@pytest.mark.parametrize("case", list(REC_MESSAGE))
@pytest.mark.parametrize("entry", list(REC_ENTRIES))
def test_record_entries_reject(nat, entry, case):
    rec, idx, affine = _records()
    lb = LB
    if case == "rec_int8":
        rec = rec.to(torch.int8)
    elif case == "idx_int32":
        idx = idx.to(torch.int32)
    elif case == "idx_len1":
        idx = idx[:1].contiguous()
    elif case == "label_bytes_0":
        lb = 0
    elif case == "label_bytes_9":
        lb = 9
    elif case == "rec_wide":
        rec = torch.cat([rec, rec[:, :1]], 1).contiguous()
    with pytest.raises(RuntimeError, match=REC_MESSAGE[case]):
        REC_ENTRIES[entry](nat, rec, idx, affine, lb)


def test_record_entries_accept(nat):
    rec, idx, affine = _records()
    x, y = REC_ENTRIES["record_decode"](nat, rec, idx, affine, LB)
    rx, ry = _ref.record_decode(rec, idx, affine, (C, H, W), 3, 2, 1, True, True, LB)
    assert torch.equal(x, rx) and torch.equal(y, ry) and y.tolist() == rec[:, 0].tolist()
    x, y = REC_ENTRIES["record_decode_rrc"](nat, rec, idx, affine, LB)
    rx, ry = _ref.record_decode_rrc(rec, idx, affine, (C, H, W), (4, 4), 3, 2, True, True, LB)
    assert torch.equal(x, rx) and torch.equal(y, ry)
    out = REC_ENTRIES["record_augment"](nat, rec, idx, affine, LB)
    assert torch.equal(out, _ref.record_augment(rec, idx, (C, H, W), 3, 2, LB))
