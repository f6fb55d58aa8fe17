"""The argument checks the Python entries share (csrc/bind/common.hpp): ``ce_args`` for the five
cross-entropy entries, ``top1_correct`` and ``eval_stats``; ``check_records`` for
``record_decode``, ``record_decode_rrc`` and ``record_augment``; and the output-extent checks of
the pools and the direct convolutions (``pool_out``, ``gconv_shape``, ``maxpool_bwd``).

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


@pytest.mark.parametrize("last", [-1, 11, V, V + 5])
def test_ce_hard_labels_outside_the_classes_accept(nat, last):
    """A hard label that is no class (and not ignore_index) is no error and reads nothing: -1,
    valid_cols (a padding column), V and V + 5, on the first rows and on the last."""
    logits, labels = _ce_inputs()
    labels = torch.tensor([-1, 11, V, last], device="cuda")
    ref_loss, ref_grad = _ref.cross_entropy_fwd_bwd(logits, labels, 0.0, -100, 11)
    loss, work = nat.cross_entropy_fwd(logits, labels, 0.0, -100, 11)
    assert int(work[0]) == R
    _close_ce(loss, nat.cross_entropy_bwd(logits, labels, work, _gout(), 0.0, -100, 11), ref_loss,
              ref_grad)
    _close_ce(*nat.cross_entropy_fwd_bwd(logits, labels, 0.0, -100, 11), ref_loss, ref_grad)
    assert torch.isfinite(loss) and not ref_grad[:, 11:].any()


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


# ------------------------------------------------------------- pooling / direct-conv geometry
# pool_out (csrc/bind/common.hpp) and gconv_shape (csrc/bindings.cpp): a padded input smaller than
# the window has no output.  H = 2, k = 3, s = 2, p = 0 once gave extent 1 (C++ division truncates
# -1 / 2 to 0) and a kernel launch over a partial window; torch raises.  H = 3 is the smallest
# valid input: a 1x1 output.  C = 8 depthwise, so dy is [1, 1, 1, 8] in both cases.
GC = 8
GEO_MESSAGE = "is smaller than the"


def _geo_x(H):
    g = torch.Generator().manual_seed(3)
    return torch.randint(-3, 4, (1, H, H, GC), generator=g).to(torch.bfloat16).cuda()


def _geo_w():
    g = torch.Generator().manual_seed(4)
    return (torch.randint(0, 2, (GC, 3, 3, 1), generator=g) * 2 - 1).to(torch.bfloat16).cuda()


def _geo_dy():
    return torch.tensor([1, -2, 3, -1, 2, -3, 1, 2]).reshape(1, 1, 1, GC).to(torch.bfloat16).cuda()


GEO_ENTRIES = {
    "maxpool_fwd": lambda c, H: c.maxpool_fwd(_geo_x(H), 3, 2, 0, False)[0],
    "avgpool2d_fwd": lambda c, H: c.avgpool2d_fwd(_geo_x(H), 3, 2, 0),
    "gconv_fwd": lambda c, H: c.gconv_fwd(_geo_x(H), _geo_w(), [2, 2], [0, 0], GC, None, 0),
    "gconv_dgrad": lambda c, H: c.gconv_dgrad(_geo_dy(), _geo_w(), [1, H, H, GC], [2, 2], [0, 0],
                                              GC, None, 0),
    "gconv_wgrad": lambda c, H: c.gconv_wgrad(_geo_dy(), _geo_x(H), 3, 3, [2, 2], [0, 0], GC, None,
                                              0, None, None, True)[0],
}


@pytest.mark.parametrize("entry", list(GEO_ENTRIES))
def test_window_larger_than_input_rejects(nat, entry):
    with pytest.raises(RuntimeError, match=GEO_MESSAGE):
        GEO_ENTRIES[entry](nat, 2)


def test_window_equal_to_input_accepts(nat):
    x, w, dy = _geo_x(3), _geo_w(), _geo_dy()
    xn = x.float().permute(0, 3, 1, 2)
    y = GEO_ENTRIES["maxpool_fwd"](nat, 3)
    assert y.shape == (1, 1, 1, GC)
    assert torch.equal(y.float(), torch.nn.functional.max_pool2d(xn, 3, 2, 0).permute(0, 2, 3, 1))
    y = GEO_ENTRIES["avgpool2d_fwd"](nat, 3)
    ref = torch.nn.functional.avg_pool2d(xn.double(), 3, 2, 0).permute(0, 2, 3, 1)
    assert y.shape == (1, 1, 1, GC)
    # one bf16 rounding of sum / 9: half an ulp, 2^-9 relative
    assert bool(((y.double() - ref).abs() <= ref.abs() * 2.0 ** -8).all())
    # integer data: the 27-term sums are exact in bf16, so the conv results equal torch's
    y = GEO_ENTRIES["gconv_fwd"](nat, 3)
    assert y.shape == (1, 1, 1, GC)
    assert torch.equal(y.float(), _ref.gconv_fwd(x.float(), w.float(), (2, 2), (0, 0), GC))
    dx = GEO_ENTRIES["gconv_dgrad"](nat, 3)
    assert torch.equal(dx.float(), _ref.gconv_dgrad(dy.float(), w.float(), (1, 3, 3, GC), (2, 2),
                                                    (0, 0), GC))
    dw = GEO_ENTRIES["gconv_wgrad"](nat, 3)
    assert torch.equal(dw, _ref.gconv_wgrad(dy.float(), x.float(), 3, 3, (2, 2), (0, 0), GC)[0])


def _pool_bwd_args(C=8):
    """A valid maxpool_bwd call: x [2, 7, 7, C], 3/2/1 -> 4x4 (floor and ceil extents agree)."""
    dy = torch.ones(2, 4, 4, C, dtype=torch.bfloat16, device="cuda")
    idx = torch.full((2, 4, 4, C), 4, dtype=torch.uint8, device="cuda")   # the window's centre
    return dy, idx, [2, 7, 7, C]


@pytest.mark.parametrize("case", ["batch", "extent", "channels"])
def test_maxpool_bwd_rejects(nat, case):
    dy, idx, xs = _pool_bwd_args(12 if case == "channels" else 8)
    if case == "batch":
        xs[0] = 3
        msg = "dy batch"
    elif case == "extent":      # 5x5 is neither the floor nor the ceil extent of 7 / 3 / 2 / 1
        dy = torch.ones(2, 5, 5, 8, dtype=torch.bfloat16, device="cuda")
        idx = torch.zeros(2, 5, 5, 8, dtype=torch.uint8, device="cuda")
        msg = "does not match the pooling geometry"
    else:
        msg = "C % 8 == 0"
    with pytest.raises(RuntimeError, match=msg):
        nat.maxpool_bwd_impl(dy, idx, xs, 3, 2, 1)


def test_maxpool_bwd_accepts(nat):
    dy, idx, xs = _pool_bwd_args()
    dx = nat.maxpool_bwd_impl(dy, idx, xs, 3, 2, 1)
    want = torch.zeros(xs)
    want[:, 0::2, 0::2, :] = 1.0      # centre of window (ho, wo) is pixel (2 ho, 2 wo)
    assert torch.equal(dx.float().cpu(), want)
    # a ceil-mode extent (8 / 3 / 2 / 0: floor 3, ceil 4) is accepted as well
    x = torch.arange(2 * 8 * 8 * 8, dtype=torch.float32).reshape(2, 8, 8, 8).to(torch.bfloat16).cuda()
    y, idx = nat.maxpool_fwd(x, 3, 2, 0, True)
    assert y.shape == (2, 4, 4, 8)
    dx = nat.maxpool_bwd_impl(torch.ones_like(y), idx, [2, 8, 8, 8], 3, 2, 0)
    assert dx.float().sum().item() == y.numel()


# --------------------------------------------------------------------------- BatchNorm, empty input
# bn.hip's apply kernels clamp their row to M - 1 and load before the bounds check, so M = 0 must
# be refused on the host: [0, 8] (no rows) and [4, 0] (no channels), bf16 and fp32.
def _bn_vec(C):
    return torch.ones(C, dtype=torch.float32, device="cuda")


def _bn_empty(shape, dtype):
    return torch.zeros(shape, dtype=dtype, device="cuda")


BN_EMPTY_ENTRIES = {
    "bn_act_fwd": lambda c, t, C: c.bn_act_fwd(t, _bn_vec(C), _bn_vec(C), True, None, None, None),
    "bn_act_fwd_residual": lambda c, t, C: c.bn_act_fwd(t, _bn_vec(C), _bn_vec(C), True, t, None,
                                                        None),
    "bn_act_bwd_reduce": lambda c, t, C: c.bn_act_bwd_reduce(t, t, t, _bn_vec(C), _bn_vec(C), True),
    "bn_act_bwd_apply": lambda c, t, C: c.bn_act_bwd_apply(
        t, t, t, _bn_vec(C), _bn_vec(C), _bn_vec(C), _bn_vec(C), _bn_vec(C), 16, True, True, None,
        None, None, None, None),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(0, 8), (4, 0)], ids=["no_rows", "no_channels"])
@pytest.mark.parametrize("entry", list(BN_EMPTY_ENTRIES))
def test_bn_entries_reject_empty(nat, entry, shape, dtype):
    with pytest.raises(RuntimeError, match="empty input"):
        BN_EMPTY_ENTRIES[entry](nat, _bn_empty(shape, dtype), shape[1])


def test_bn_entries_accept_one_row(nat):
    """The smallest valid input, [1, 8] of ones with unit vectors: z = 2, the sums are 1 and 0."""
    t = torch.ones(1, 8, dtype=torch.bfloat16, device="cuda")
    z = BN_EMPTY_ENTRIES["bn_act_fwd"](nat, t, 8)
    assert z.shape == (1, 8) and bool((z == 2).all())
    sg, sgx, sgx2 = BN_EMPTY_ENTRIES["bn_act_bwd_reduce"](nat, t, 8)
    assert sg.tolist() == [1.0] * 8 and sgx.tolist() == [0.0] * 8 and sgx2 is None
    dy, dres = BN_EMPTY_ENTRIES["bn_act_bwd_apply"](nat, t, 8)
    # dy = 1 * (g - 1/16 - 0 * 1/16) with g = 1
    assert dy.float().tolist() == [[0.9375] * 8] and bool((dres == 1).all())
