"""loss.hip on the MI355X at its launch edges: the split pair (cross_entropy_fwd + _bwd), the
fused cross_entropy_fwd_bwd, the pair-target entries and top1_correct against the float64
reference of tests/ce_common.py, per element, with the bounds derived there.  Shapes come from the
exported launch constants (CE_THREADS, CE_VEC, CE_BWD_MAX_GRID_ROWS, TOP1_ROWS_PER_BLOCK); each
test asserts the edge it crosses.  The reference runs in torch float64 on the same device.

Every test prints the running maxima of error / bound.

Labels outside the classes are fed to the kernels here: they read nothing (ce_label_logit in
loss.hip guards every label read)."""
from types import SimpleNamespace

import pytest
import torch

import ce_common as cc

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
WORST = {}          # (output, dtype id) -> (ratio, where): printed by every test that updates it


@pytest.fixture(autouse=True)
def _native():
    from mipipe.ops._native import load_error, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"


def C():
    from mipipe.ops._native import native
    return native()


def K():
    return cc.consts_of(C())


_REFS = {}


def _ref(case, eps, dtype):
    key = (case.name, dtype, eps)
    if key not in _REFS:
        if len(_REFS) > 64:
            _REFS.clear()
        _REFS[key] = cc.ref64(case.x.cuda(), case.labels.cuda(), eps, case.valid_cols, case.lam,
                              k=K())
    return _REFS[key]


def _mix(lam):
    return torch.tensor([lam, 1, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")


def run_split(case, eps, gout):
    """(loss, grad, count, row losses, row lse) of the split form, hard or pair-target."""
    x, labels = case.x.cuda(), case.labels.cuda()
    R = x.shape[0]
    g = torch.tensor([gout], dtype=torch.float32, device="cuda")
    if case.lam is None:
        loss, work = C().cross_entropy_fwd(x, labels, eps, cc.IGNORE, case.valid_cols)
        grad = C().cross_entropy_bwd(x, labels, work, g, eps, cc.IGNORE, case.valid_cols)
        count = int(work[0])
    else:
        mix = _mix(case.lam)
        loss, work = C().cross_entropy_mixed_fwd(x, labels, mix, eps, case.valid_cols)
        grad = C().cross_entropy_mixed_bwd(x, labels, mix, work, g, eps, case.valid_cols)
        count = None                                    # every row counts: nothing is counted
    assert work.shape == (4 + 2 * R,) and loss.dtype == torch.float32 and grad.dtype == x.dtype
    return SimpleNamespace(loss=loss, grad=grad, count=count, work=work,
                           rowloss=work[4:4 + R].view(torch.float32),
                           lse=work[4 + R:].view(torch.float32))


def run_fused(case, eps):
    loss, grad = C().cross_entropy_fwd_bwd(case.x.cuda(), case.labels.cuda(), eps, cc.IGNORE,
                                           case.valid_cols)
    return SimpleNamespace(loss=loss, grad=grad, count=None, rowloss=None, lse=None)


def _note(r, dtype, where):
    for key, v in r.items():
        k2 = (key, cc.DT_ID[dtype])
        if v > WORST.get(k2, (0.0, ""))[0]:
            WORST[k2] = (v, where)


def check(case, eps, gout, dtype):
    """Every form that applies to the case, against float64.  The fused form has no upstream
    gradient: it runs with gout = 1."""
    ref = _ref(case, eps, dtype)
    out = run_split(case, eps, gout)
    _note(cc.compare(case, eps, gout, out, ref, dtype), dtype, f"{case.name} eps={eps} split")
    if case.lam is None and gout == 1.0:
        out = run_fused(case, eps)
        _note(cc.compare(case, eps, 1.0, out, ref, dtype), dtype, f"{case.name} eps={eps} fused")
    return ref


def _report():
    print("worst error / bound so far: " +
          ", ".join(f"{k[0]} {k[1]} {v:.3f} ({w})" for k, (v, w) in sorted(WORST.items())))


def grid3(fn):
    fn = pytest.mark.parametrize("gout", cc.GOUT_LIST)(fn)
    fn = pytest.mark.parametrize("eps", cc.EPS_LIST)(fn)
    return pytest.mark.parametrize("dtype", DTYPES, ids=IDS)(fn)


# ------------------------------------------------------------------------------ column edges
@grid3
def test_column_edges_vector(dtype, eps, gout):
    k = K()
    item = k.threads * k.vec
    cases = cc.column_cases_vector(dtype, k.threads, k.vec)
    vs = sorted({c.x.shape[1] for c in cases})
    # one item; one short of, exactly and one past an item per thread (the last: a second trip of
    # the forward and a second ce_bwd column block with one live thread); two trips + 1
    assert vs == [k.vec, item - k.vec, item, item + k.vec, 2 * item + k.vec]
    assert -(-(item + k.vec) // k.vec // k.threads) == 2
    seen = set()
    for case in cases:
        V = case.x.shape[1]
        Vv = cc.classes(V, case.valid_cols)
        assert V % k.vec == 0
        seen.add("all" if Vv == V else "cut" if Vv % k.vec else "whole")
        if Vv == 5:
            assert V == item and Vv < k.vec      # lanes 1.. and waves 1..3 see no class at all
        ref = check(case, eps, gout, dtype)
        if Vv == 1 and eps == 0.0 and case.lam is None:
            assert float(ref.loss) == 0.0 and not ref.grad.any()
            out = run_split(case, eps, gout)
            assert float(out.loss) == 0.0 and not out.grad.any(), case.name
    assert seen == {"all", "cut", "whole"}
    _report()


@grid3
def test_column_edges_scalar(dtype, eps, gout):
    k = K()
    cases = cc.column_cases_scalar(dtype, k.threads, k.vec)
    assert sorted({c.x.shape[1] for c in cases}) == \
        [1, 7, k.threads - 1, k.threads, k.threads + 1, 2 * k.threads + 1, 1001]
    for case in cases:
        check(case, eps, gout, dtype)
    _report()


# ------------------------------------------------------------------------------ row edges
@grid3
def test_row_edges_of_count_and_sum(dtype, eps, gout):
    """ce_count_kernel / ce_sum_kernel are one block striding over the rows: R around one and two
    trips, under every ignore pattern; work[0] is the valid count exactly (asserted in compare)."""
    k = K()
    cases = cc.row_cases(dtype, k.threads)
    assert sorted({c.x.shape[0] for c in cases}) == \
        [1, 2, 3, k.threads - 1, k.threads, k.threads + 1, 2 * k.threads + 1]
    for case in cases:
        ref = check(case, eps, gout, dtype)
        if case.name.endswith("ignore=all"):
            assert ref.count == 0 and ref.n == 1
            out = run_split(case, eps, gout)
            assert out.count == 0 and float(out.loss) == 0.0 and not out.grad.any(), case.name
            fused = run_fused(case, eps)
            assert float(fused.loss) == 0.0 and not fused.grad.any(), case.name
        if case.name.endswith("only_last_valid"):
            assert ref.count == 1
    _report()


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@grid3
def test_row_edges_of_bwd_grid(dtype, eps, gout, which):
    """ce_bwd's grid.y is capped: a block's row loop takes a second (third) trip past the cap.
    Every element of every row is compared; the first rows and the rows past the cap are looked
    at again on their own, so that a failure names its region."""
    k = K()
    cap = k.bwd_max_grid_rows
    R = (cap, cap + 1, cap + 2, 2 * cap + 1)[which]
    cases = [c for c in cc.grid_row_cases(dtype, cap, k.vec) if c.x.shape[0] == R]
    assert len(cases) == 4 and {c.x.shape[1] for c in cases} == {k.vec, k.vec - 1}
    assert (R > cap) == (which > 0) and (R > 2 * cap) == (which == 3)
    assert R * k.vec <= 131071 * 8
    for case in cases:
        ref = check(case, eps, gout, dtype)
        out = run_split(case, eps, gout)
        g, g64 = out.grad.double(), cc.scale_grad(ref, gout)
        tol = 2.0 ** -7 * g64.abs() + 2.0 ** -14 / ref.n    # coarse; compare() holds the bound
        for name, rows in (("first", slice(0, 64)), ("last", slice(max(0, R - cap - 2), R))):
            bad = ((g[rows] - g64[rows]).abs() > tol[rows]).nonzero()
            assert bad.numel() == 0, f"{case.name}: {name} rows differ at {bad[:4].tolist()}"
    _report()


# ------------------------------------------------------------------------------ labels, pair targets
@grid3
def test_labels_outside_the_classes(dtype, eps, gout):
    """-1, Vv, V and V + 5, on rows that are not the last and on the last: the logit counts as
    0, no column gets the target, the row counts in n."""
    for case in cc.label_cases(dtype):
        V = case.x.shape[1]
        Vv = cc.classes(V, case.valid_cols)
        lab = case.labels
        outside = (lab != cc.IGNORE) & ((lab < 0) | (lab >= Vv))
        assert outside[:-1].any() and outside[-1]
        ref = check(case, eps, gout, dtype)
        assert ref.n == (7 if case.lam is None else 8)
    _report()


@grid3
def test_pair_target(dtype, eps, gout):
    seen = set()
    for case in cc.pair_cases(dtype):
        R = case.x.shape[0]
        check(case, eps, gout, dtype)
        seen.add((R, case.lam))
        if case.lam == 1.0:             # the hard-label kernels' bits (labels outside included)
            hard = SimpleNamespace(**{**vars(case), "lam": None})
            a, b = run_split(case, eps, gout), run_split(hard, eps, gout)
            assert torch.equal(a.loss, b.loss) and torch.equal(a.grad, b.grad), case.name
            assert torch.equal(a.work[4:], b.work[4:]), case.name
    assert seen == {(R, lam) for R in (1, 2, 3, 256, 257) for lam in (0.0, 1.0, 0.5, 0.3)}
    _report()


# ------------------------------------------------------------------------------ magnitude, exact
@grid3
def test_magnitude(dtype, eps, gout):
    for case in cc.magnitude_cases(dtype):
        check(case, eps, gout, dtype)
    _report()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases(dtype):
    for case in cc.exact_cases(dtype):
        Vv = cc.classes(case.x.shape[1], case.valid_cols)
        n = max(1, int((case.labels != cc.IGNORE).sum()))
        assert Vv & (Vv - 1) == 0 and n & (n - 1) == 0
        out = run_fused(case, 0.0)
        want = cc.exact_grad(case).cuda()
        assert torch.equal(out.grad.double(), want), case.name
        check(case, 0.0, 1.0, dtype)


# ------------------------------------------------------------------------------ non-finite logits
@grid3
def test_nonfinite_logits(dtype, eps, gout):
    """-inf in non-label class columns at eps = 0: a finite loss within its bound, gradient 0
    there, the rest within bound (all asserted in compare).  +inf / NaN rows, and -inf under
    smoothing: the outputs that are finite are those of the reference."""
    for case in cc.nonfinite_cases(dtype):
        ref = check(case, eps, gout, dtype)
        if "-inf" in case.name and eps == 0.0:
            out = run_split(case, eps, gout)
            assert torch.isfinite(out.loss) and torch.isfinite(ref.loss), case.name
            assert torch.isfinite(out.grad).all(), case.name
            if case.lam is None:
                fused = run_fused(case, eps)
                assert torch.isfinite(fused.loss) and torch.isfinite(fused.grad).all(), case.name
        if "padding" in case.name:
            assert torch.isfinite(ref.loss)
    _report()


# ------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("lam", [None, 0.3], ids=["hard", "pair"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_launches_same_bits(dtype, lam):
    k = K()
    case = cc._random("det", 2 * k.threads + 1, 1000, -1, dtype, lam,
                      ignore=(3, 77) if lam is None else ())
    a, b = run_split(case, 0.1, 0.37), run_split(case, 0.1, 0.37)
    assert torch.equal(a.loss, b.loss) and torch.equal(a.grad, b.grad)
    assert torch.equal(a.work[4:], b.work[4:]) and a.count == b.count
    if lam is None:
        fa, fb = run_fused(case, 0.1), run_fused(case, 0.1)
        assert torch.equal(fa.loss, fb.loss) and torch.equal(fa.grad, fb.grad)


@pytest.mark.parametrize("V", [1000, 1001])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_appended_rows_leave_the_first_rows_bits(dtype, V):
    """Rows [0, 256) of the gradient do not depend on how many rows follow (the appended rows are
    ignored, so n stays): no row's result leans on the grid's shape."""
    k = K()
    base = cc._random("append", k.threads, V, -1, dtype, None, ignore=(5,))
    g0 = run_split(base, 0.1, 0.37).grad
    f0 = run_fused(base, 0.1).grad
    for extra in (1, k.threads + 1):
        more = cc._random("append+", extra, V, -1, dtype, None, ignore=range(extra), seed=1)
        case = SimpleNamespace(name="appended", x=torch.cat([base.x, more.x]),
                               labels=torch.cat([base.labels, more.labels]), valid_cols=-1,
                               lam=None)
        out = run_split(case, 0.1, 0.37)
        assert out.count == k.threads - 1
        assert torch.equal(out.grad[:k.threads], g0) and not out.grad[k.threads:].any()
        assert torch.equal(run_fused(case, 0.1).grad[:k.threads], f0)


# ------------------------------------------------------------------------------ top-1
def _eval_stats_top1(x, labels):
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    C().eval_stats(x, labels, counters, None, None, 1, cc.IGNORE, -1)
    return int(counters[1])


@pytest.mark.parametrize("R", cc.TOP1_R)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_top1_correct(dtype, R):
    k = K()
    rows = k.top1_rows
    assert cc.TOP1_R == (1, rows - 1, rows, rows + 1, 1021) and 1021 % rows == 1
    for V in cc.TOP1_V:
        for start in cc.top1_starts(R, V):
            x, labels = cc.top1_case(dtype, R, V, start)
            want = cc.top1_ref(x, labels)
            xg, lg = x.cuda(), labels.cuda()
            got = C().top1_correct(xg, lg)
            assert got.dtype == torch.int32 and int(got) == want, (R, V, start, int(got), want)
            # accumulation into a counter that already holds something
            acc = torch.tensor([41], dtype=torch.int32, device="cuda")
            assert C().top1_correct(xg, lg, acc) is acc and int(acc) == 41 + want
            # the other evaluation kernel counts the same rows
            assert _eval_stats_top1(xg, lg) == want, (R, V, start)


def test_top1_special_rows_by_hand():
    """The rows of the contract one at a time, with the answer written down."""
    INF, NAN = cc.INF, cc.NAN
    V = 130
    def row(**at):
        x = torch.full((V,), -2.0)
        for c, v in at.items():
            x[int(c[1:])] = v
        return x
    table = [
        (torch.full((V,), -INF), 0, 1), (torch.full((V,), -INF), 1, 0),
        (row(c0=4.0, c64=4.0), 0, 1), (row(c0=4.0, c64=4.0), 64, 0),     # within one lane
        (row(c3=4.0, c4=4.0), 3, 1), (row(c3=4.0, c4=4.0), 4, 0),         # across lanes
        (row(c129=9.0), 129, 1), (row(c0=9.0), 0, 1),
        (row(c5=INF, c70=INF), 5, 1), (row(c5=INF, c70=INF), 70, 0),
        (row(c0=NAN, c1=50.0), 0, 1), (row(c1=50.0, c129=NAN), 129, 1),
        (row(c7=NAN, c90=NAN), 7, 1), (row(c7=NAN, c90=NAN), 90, 0),
        (row(c0=3.0), cc.IGNORE, 0), (row(c0=3.0), V, 0),
    ]
    for dtype in DTYPES:
        for x, y, want in table:
            xs, ys = x[None].to(dtype), torch.tensor([y])
            assert cc.top1_ref(xs, ys) == want
            assert int(C().top1_correct(xs.cuda(), ys.cuda())) == want, (dtype, y, want)
            assert _eval_stats_top1(xs.cuda(), ys.cuda()) == want, (dtype, y, want)
