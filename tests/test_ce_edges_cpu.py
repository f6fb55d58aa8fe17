"""The design of the cross-entropy / top-1 edge tests, proven without a GPU (tests/ce_common.py):
the float64 reference equals torch's float64 cross-entropy, the exact constructions are exact, the
shipped CPU reference and the fp32 model of the kernels' arithmetic sit inside every bound (the
model at or below half), and every defect switch is caught by the comparison the GPU file uses."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import ce_common as cc
from mipipe.ops import _ref

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _in_range(case):
    Vv = cc.classes(case.x.shape[1], case.valid_cols)
    lab = case.labels
    ok = (lab >= 0) & (lab < Vv)
    if case.lam is None:
        ok |= lab == cc.IGNORE
    return bool(ok.all())


def _finite(case):
    Vv = cc.classes(case.x.shape[1], case.valid_cols)
    return bool(torch.isfinite(case.x[:, :Vv].float()).all())


def _small_cases(dtype):
    return cc.all_cases(dtype, big=False)


# ------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("eps", cc.EPS_LIST)
def test_reference_equals_torch_float64(eps):
    """Hard labels: F.cross_entropy in float64 with ignore_index and label_smoothing, autograd
    gradients times gout.  Pair targets: its probability-target form on the class columns."""
    gout = 0.37
    seen = {"hard": 0, "pair": 0}
    for case in _small_cases(torch.float32) + cc.grid_row_cases(torch.float32)[:2]:
        if not (_in_range(case) and _finite(case)):
            continue
        R, V = case.x.shape
        Vv = cc.classes(V, case.valid_cols)
        ref = cc.ref64(case.x, case.labels, eps, case.valid_cols, case.lam)
        x = case.x[:, :Vv].double().requires_grad_(True)
        if case.lam is None:
            if ref.count == 0:
                continue                    # torch: 0 / 0
            loss = F.cross_entropy(x, case.labels, ignore_index=cc.IGNORE,
                                   label_smoothing=cc.f32(eps))
            seen["hard"] += 1
        else:
            a, b = case.labels, case.labels.flip(0)
            lam = cc.f32(case.lam)
            tgt = lam * F.one_hot(a, Vv).double() + (1 - lam) * F.one_hot(b, Vv).double()
            loss = F.cross_entropy(x, tgt, label_smoothing=cc.f32(eps))
            seen["pair"] += 1
        (loss * cc.f32(gout)).backward()
        assert abs(loss.item() - ref.loss.item()) <= 1e-12 * max(1.0, abs(loss.item())), case.name
        g = cc.scale_grad(ref, gout)
        scale = x.grad.abs().max().item() + 1e-300
        assert (g[:, :Vv] - x.grad).abs().max().item() <= 1e-12 * max(scale, 1e-6), case.name
        assert not g[:, Vv:].any(), case.name
    assert seen["hard"] > 100 and seen["pair"] > 60, seen


def test_reference_out_of_range_labels_by_hand():
    """A label outside the classes: the row's loss is its lse (plus smoothing), softmax - eps/Vv
    is its gradient, and it counts in n."""
    x = torch.tensor([[0.0, 1.0, 2.0, 50.0], [1.0, 1.0, 1.0, 50.0]])
    lab = torch.tensor([3, 1])
    ref = cc.ref64(x, lab, 0.0, valid_cols=3)
    lse0 = torch.logsumexp(x[0, :3].double(), 0)
    lse1 = torch.logsumexp(x[1, :3].double(), 0)
    assert ref.n == 2 and abs(ref.loss.item() - ((lse0 - 0.0) + (lse1 - 1.0)).item() / 2) < 1e-15
    assert torch.allclose(ref.grad[0, :3], torch.softmax(x[0, :3].double(), 0) / 2, atol=1e-16)
    assert not ref.grad[:, 3].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_top1_reference_equals_argmax(dtype):
    for R in cc.TOP1_R:
        for V in cc.TOP1_V:
            for start in cc.top1_starts(R, V):
                x, labels = cc.top1_case(dtype, R, V, start)
                clean = ~torch.isnan(x.float()).any(1)
                want = int((x[clean].float().argmax(1) == labels[clean]).sum())
                assert cc.top1_ref(x[clean], labels[clean]) == want, (R, V, start)
    # NaN rows by hand: the first NaN is the top-1 index
    x = torch.tensor([[1.0, cc.NAN, 7.0, cc.NAN], [cc.NAN, 9.0, 1.0, 2.0], [3.0, 9.0, 1.0, cc.NAN]])
    assert cc.top1_ref(x, torch.tensor([1, 0, 3])) == 3
    assert cc.top1_ref(x, torch.tensor([3, 1, 1])) == 0
    assert cc.top1_ref(torch.full((2, 5), -cc.INF), torch.tensor([0, 1])) == 1


# ------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases_are_exact(dtype):
    """The exact gradient is representable in the logits' type, equals the float64 reference, and
    the fp32 model of the fused kernel reaches it bit for bit."""
    for case in cc.exact_cases(dtype):
        R, V = case.x.shape
        Vv = cc.classes(V, case.valid_cols)
        n = max(1, int((case.labels != cc.IGNORE).sum()))
        assert Vv & (Vv - 1) == 0 and n & (n - 1) == 0, case.name
        g = cc.exact_grad(case)
        assert torch.equal(g.to(dtype).double(), g), case.name
        ref = cc.ref64(case.x, case.labels, 0.0, case.valid_cols)
        assert (ref.grad - g).abs().max().item() <= 2.0 ** -50, case.name
        m = cc.model32(case.x, case.labels, 0.0, 1.0, case.valid_cols, fused=True)
        assert torch.equal(m.grad.double(), g), case.name


# ------------------------------------------------------------------------------ inside the bounds
def _shipped(case, eps, gout):
    """The shipped CPU reference evaluated in fp32, as ``compare`` takes it."""
    x32 = case.x.float()
    if case.lam is None:
        loss, g = _ref.cross_entropy_fwd_bwd(x32, case.labels, eps, cc.IGNORE, case.valid_cols)
    else:
        mix = torch.tensor([case.lam, 1, 0, 0, 0, 0, 0, 0], dtype=torch.float32)
        loss, g = _ref.cross_entropy_mixed_fwd_bwd(x32, case.labels, mix, eps, case.valid_cols)
    return SimpleNamespace(loss=loss, grad=g.double() * gout, count=None, rowloss=None, lse=None)


@pytest.mark.parametrize("eps", cc.EPS_LIST)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shipped_reference_and_model_inside_bounds(dtype, eps):
    worst = {}
    big = cc.grid_row_cases(dtype)
    for case in _small_cases(dtype) + [big[0], big[1], big[-2], big[-1]]:
        ref = cc.ref64(case.x, case.labels, eps, case.valid_cols, case.lam)
        for gout in cc.GOUT_LIST:
            # the shipped reference computes in fp32 whatever the logits' type: fp32 bounds
            cc.compare(case, eps, gout, _shipped(case, eps, gout), ref, torch.float32)
            forms = (False, True) if (case.lam is None and gout == 1.0) else (False,)
            for fused in forms:
                out = cc.model32(case.x, case.labels, eps, gout, case.valid_cols, case.lam, fused)
                if fused:
                    out.lse = out.count = None
                r = cc.compare(case, eps, gout, out, ref, dtype)
                for key, v in r.items():
                    if v > worst.get(key, (0.0, ""))[0]:
                        worst[key] = (v, case.name)
                    # (the whole gradient, target columns included: ce_common's docstring)
                    assert v <= (1.0 if key == "grad" else 0.5), (case.name, eps, gout, fused, key, v)
    print(f"model32 {cc.DT_ID[dtype]} eps={eps}: " +
          ", ".join(f"{k} {v:.3f} ({n})" for k, (v, n) in sorted(worst.items())))


# ------------------------------------------------------------------------------ the defects
def _as_out(ref, gout, dtype):
    return SimpleNamespace(loss=ref.loss, grad=cc.scale_grad(ref, gout).to(dtype), count=ref.count,
                           rowloss=ref.rowloss.float(), lse=ref.lse.float())


def _fails(case, eps, gout, defect, dtype=torch.float32):
    ref = cc.ref64(case.x, case.labels, eps, case.valid_cols, case.lam)
    bad = cc.ref64(case.x, case.labels, eps, case.valid_cols, case.lam, defect=defect)
    cc.compare(case, eps, gout, _as_out(ref, gout, dtype), ref, dtype)   # the true one passes
    try:
        cc.compare(case, eps, gout, _as_out(bad, gout, dtype), ref, dtype)
    except AssertionError:
        return True
    return False


# Cases that no defect switch can fail at (eps, gout) = (0.1, 0.37), and what they are there for:
#  * every row ignored (at R = 1 "one" and "every second" are that too): the loss and every gradient element are exactly 0 whatever n is taken to
#    be; they pin "count 0, n clamps to 1, loss exactly 0, gradient all zero";
#  * one column that is the one class (V = Vv = 1): softmax and target are both 1, the loss and
#    the gradient are 0; it is the smallest shape the scalar path can be launched with.
BLIND = {f"rows R={R} ignore=all" for R in (1, 2, 3, 255, 256, 257, 513)} | \
    {"rows R=1 ignore=one", "rows R=1 ignore=every_second"} | \
    {"scalar V=1 Vv=1 hard", "scalar V=1 Vv=1 pair"}


def test_every_defect_fails_a_case_and_blind_cases_are_known():
    caught = {d: 0 for d in cc.DEFECTS}
    blind = set()
    for case in _small_cases(torch.float32):
        hit = False
        for d in cc.DEFECTS:
            if d == "rows_past_grid_cap_unwritten":
                continue                    # needs R past the cap: below
            if _fails(case, 0.1, 0.37, d):
                caught[d] += 1
                hit = True
        if not hit:
            blind.add(case.name)
    for case in cc.grid_row_cases(torch.float32):
        R = case.x.shape[0]
        fails = _fails(case, 0.1, 0.37, "rows_past_grid_cap_unwritten")
        assert fails == (R > cc.CPU_CONSTS.bwd_max_grid_rows), case.name
        caught["rows_past_grid_cap_unwritten"] += fails
    assert all(caught.values()), caught
    assert blind == BLIND, (sorted(blind - BLIND), sorted(BLIND - blind))
    # a defect of the smoothing alone is invisible without smoothing: eps = 0 runs beside 0.1
    case = cc.column_cases_vector(torch.float32)[2]
    assert not _fails(case, 0.0, 1.0, "smooth_mean_all_cols")
    print({d: n for d, n in caught.items()})


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_top1_defect_fails_a_case(dtype):
    for d in cc.TOP1_DEFECTS:
        n = 0
        for R in cc.TOP1_R:
            for V in cc.TOP1_V:
                for start in cc.top1_starts(R, V):
                    x, labels = cc.top1_case(dtype, R, V, start)
                    n += cc.top1_ref(x, labels) != cc.top1_ref(x, labels, defect=d)
        assert n > 0, d


def test_only_the_large_magnitude_cases_waive_the_whole_tensor_ceiling():
    """Every case asserts the old whole-tensor gradient limit except the ones whose logits reach
    30 and more (ce_common's docstring): exactly these."""
    for dtype in DTYPES:
        waived = sorted(c.name for c in cc.all_cases(dtype) if not c.ceiling)
        want = sorted(f"mag V={V} {what}" for V in (1000, 257) for what in
                      ("randn*30", "randn*100", "randn*100 pair", "dominant +80", "one -80",
                       "constant -10000.0"))
        assert waived == want
        for c in cc.all_cases(dtype):
            big = float(c.x.float().nan_to_num(0.0, 0.0, 0.0).abs().max())
            assert c.ceiling == (big < 30) or "padding" in c.name, (c.name, big)


def test_case_shapes_cross_their_edges():
    """The builders' shapes, stated against the launch constants they are derived from."""
    k = cc.CPU_CONSTS
    item = k.threads * k.vec
    vs = sorted({c.x.shape[1] for c in cc.column_cases_vector(torch.float32)})
    assert vs == [8, 2040, 2048, 2056, 4104] and item == 2048
    assert cc.vector_valid_cols(2048) == [2048, 2047, 2041, 2040, 9, 5, 1]
    assert sorted({c.x.shape[1] for c in cc.column_cases_scalar(torch.float32)}) == \
        [1, 7, 255, 256, 257, 513, 1001]
    assert sorted({c.x.shape[0] for c in cc.row_cases(torch.float32)}) == \
        [1, 2, 3, 255, 256, 257, 513]
    rs = sorted({c.x.shape[0] for c in cc.grid_row_cases(torch.float32)})
    assert rs == [k.bwd_max_grid_rows, k.bwd_max_grid_rows + 1, k.bwd_max_grid_rows + 2,
                  2 * k.bwd_max_grid_rows + 1] and rs[-1] == 131071
