"""Shared by the cross-entropy / top-1 edge tests (CPU: test_ce_edges_cpu.py, GPU:
test_ce_edges_gpu.py): a float64 reference written from the definition (independent of
``mipipe.ops._ref``) with switchable defects, an fp32 model of loss.hip's arithmetic, the case
builders and the per-element error bounds.  Imports no GPU.

The contract (csrc/kernels/loss.hip, launchers.hpp).  Logits ``x`` [R, V] of which the first
``Vv`` columns are classes.  With ``m = max_c x_c`` and ``lse = m + log sum_c exp(x_c - m)`` over
the classes (so a row with a +inf or NaN logit has ``lse`` = NaN, as torch's log_softmax has),

    row loss  l = (1-eps) (lse - sum_c w_c x_c) + [eps > 0] eps (lse - mean_{c<Vv} x_c)
    target    t_c = eps / Vv + (1-eps) w_c
    gradient  g_c = (exp(x_c - lse) - t_c) gout / n   on class columns of counted rows, else 0
    loss      = sum of l over counted rows / n

* hard labels: ``w`` is one-hot at the label; rows whose label is ``ignore_index`` are not
  counted; ``n`` = number of counted rows, at least 1.
* pair targets: ``w = lam [c == a] + (1-lam) [c == b]``, ``a = labels[r]``, ``b = labels[R-1-r]``;
  every row counts, ``n = R``.
* a label outside ``[0, Vv)`` (and not ``ignore_index``) matches no column: its logit counts as 0,
  no column gets its target weight, the row still counts.
* a column with ``w_c == 0`` enters ``sum w x`` with 0 whatever its logit (a masked class, -inf).
* top-1: NaN ranks above every number, the first maximal index wins (a row of -inf only: index 0).

Bounds, per element, never whole-tensor.  ``gs = |gout| / n``, ``p`` the float64 softmax,
``A = |x| + |lse| + 16`` (a -inf logit counts as 0 in ``A``: its ``p`` is exactly 0):

    gradient, fp32 logits   |g - g64|   <= gs (p A 2^-22 + t 2^-22) + 2^-60
    gradient, bf16 logits   ... + |g64| 2^-7         (one bf16 ulp of the stored value)
    row lse                 |lse - l64| <= (|l64| + max_c |x_c| + 16) 2^-22
    row loss (work)         |l/n - ..|  <= (|l64| + |sum w x| + [eps>0] |mean x| + 16) 2^-21 / n
    loss                    the sum of the row-loss bounds + |loss64| 2^-20 (the fixed-order sum)

They follow the arithmetic: ``__expf(d)`` is ``v_exp_f32(d log2e)``, relative error about
``(1 + |d|) 2^-23``; an absolute error of ``lse`` of about ``(|lse| + |x|) 2^-24`` is a relative
error of ``p``; ``t`` is rounded once.  ``model32`` evaluates the kernels' formulas in
torch.float32 (``exp2((x - lse) log2e)``; target, scale and loss expression as in the source); the
CPU test keeps it at or below half of every bound, with one exception that the arithmetic
explains.  Where the target outweighs the softmax (``t > p A``: a label column, or any column
under smoothing, with a small ``p``) the value is ``-t gs`` and its bound ``4 * 2^-24 t gs``,
while a correct evaluation rounds up to five times there (``1 - eps``, ``eps/Vv + ..``, ``p - t``,
``gs = gout / n`` unless n is a power of two, the product): the model reaches 0.70 of the bound
on such elements (0.59 at eps = 0), and by this count a correct evaluation could in principle
pass the bound there (5 against 4 half-ulps).  The bound is kept as it is all the same: it is the
stricter choice for the kernel, and the model and the kernel stay inside it.  The rule that the
model stays at or below half of a bound is knowingly waived for the ``t`` term; the half is
asserted where the ``p A`` term decides (``p A >= t``).

The older whole-tensor limits (``max|d| / max|ref|`` below 1e-5 for fp32 and 1e-2 for bf16 logits,
1e-4 relative on the loss) stay as ceilings that every case meets as well, except the magnitude
cases whose logits reach 30 and more (``randn * 30``, ``randn * 100``, the +80 / -80 rows, the
constant -1e4 rows: their builders set ``ceiling=False``, and the CPU test pins that list).  There
the fp32 gradient bound ``gs p A 2^-22`` is itself above ``1e-5 gs`` (``A > 42``): an error of
``lse`` of half an ulp at 300 is 1.5e-5 relative in ``p``, so no fp32 evaluation keeps the old
limit.  The ratio is ``max|d| / max|g64|`` without an additive guard (a gradient that is all zero
must be met exactly).  The loss ceiling is relative to
``|loss64|``; it is asserted while the loss has not cancelled, ``|loss64| >= 2^-6`` of the mean
``|lse| + |sum w x|`` of its rows (a dominant logit of +80 gives a loss of 1e-32 from terms of
80: no fp32 evaluation is relative to that).
"""
import functools
import math
from types import SimpleNamespace

import torch

IGNORE = -100
INF = float("inf")
NAN = float("nan")
LOG2E = 1.4426950408889634

# The launch constants of launchers.hpp as this file was written.  Only the CPU test uses them (it
# has no extension to ask); the GPU test reads the exported values (consts_of).
CPU_CONSTS = SimpleNamespace(threads=256, vec=8, bwd_max_grid_rows=65535, top1_rows=4)

DT_ID = {torch.bfloat16: "bf16", torch.float32: "fp32"}
EPS_LIST = (0.0, 0.1)
GOUT_LIST = (1.0, 0.37)

DEFECTS = ("softmax_all_cols", "smooth_mean_all_cols", "ignored_rows_counted",
           "partner_same_row", "padding_minus_t", "gout_dropped", "rows_past_grid_cap_unwritten",
           "partial_vector_whole")
TOP1_DEFECTS = ("last_index_ties", "nan_not_maximal")


def consts_of(mod):
    """The exported launch constants of the extension, in CPU_CONSTS' names."""
    return SimpleNamespace(threads=mod.CE_THREADS, vec=mod.CE_VEC,
                           bwd_max_grid_rows=mod.CE_BWD_MAX_GRID_ROWS,
                           top1_rows=mod.TOP1_ROWS_PER_BLOCK)


def f32(v):
    """The fp32 value the kernels receive for a Python float (smoothing, lambda, gout): the
    reference starts from what the kernel is given, so that input rounding is no kernel error."""
    return float(torch.tensor(v, dtype=torch.float32))


def classes(V, valid_cols):
    """The kernels' Vv: valid_cols clamped to [1, V]; <= 0 means all columns."""
    return min(valid_cols, V) if valid_cols > 0 else V


# ------------------------------------------------------------------------------ float64 reference
def ref64(x, labels, eps, valid_cols=-1, lam=None, defect=None, k=CPU_CONSTS):
    """Float64 reference for an upstream gradient of 1 (the gradient is linear in gout: callers
    scale ``grad``), computed on ``x``'s device (plain torch float64 either way).  ``lam`` None:
    hard labels, else the pair-target form.  Returns a namespace:
    loss, grad [R, V], lse [R], rowloss [R] (already divided by n), count (non-ignored rows), n,
    and what the bounds need: p, t [R, Vv], wx, meanx, counted [R], xabs [R, Vv]."""
    R, V = x.shape
    Vv = classes(V, valid_cols)
    xd = x.double()
    eps = f32(eps)
    lam = None if lam is None else f32(lam)
    Vs = Vm = Vg = Vv                      # columns of the softmax / the smoothing mean / the gradient
    if defect == "softmax_all_cols":
        Vs = V
    if defect == "smooth_mean_all_cols":
        Vm = V
    if defect == "partial_vector_whole" and V % k.vec == 0:
        Vs = Vm = Vg = min(V, -(-Vv // k.vec) * k.vec)
    cols = torch.arange(V, device=x.device)
    lab = labels.long()

    def onehot(l):                          # a label outside the classes matches no column
        inside = (l >= 0) & (l < Vv)
        return ((cols[None, :] == l[:, None]) & inside[:, None]).double()

    if lam is None:
        counted = lab != IGNORE
        w = onehot(lab) * counted[:, None]
        count = int(counted.sum())
        n = max(1, R if defect == "ignored_rows_counted" else count)
    else:
        counted = torch.ones(R, dtype=torch.bool, device=x.device)
        partner = lab if defect == "partner_same_row" else lab.flip(0)
        w = lam * onehot(lab) + (1.0 - lam) * onehot(partner)
        count = R
        n = max(1, R)
    xs = xd[:, :Vs]
    m = xs.max(1).values
    m = torch.where(torch.isnan(xs).any(1), torch.full_like(m, NAN), m)
    m0 = torch.where(m == -INF, torch.zeros_like(m), m)
    lse = m + torch.log(torch.exp(xs - m0[:, None]).sum(1))
    zero = torch.zeros_like(xd)
    wx = torch.where(w != 0, w * xd, zero).sum(1)
    meanx = xd[:, :Vm].sum(1) / Vm
    row = (1.0 - eps) * (lse - wx)
    if eps > 0:
        row = row + eps * (lse - meanx)
    row = torch.where(counted, row, torch.zeros_like(row))
    loss = row.sum() / n
    t = eps / Vv + (1.0 - eps) * w
    p = torch.exp(xd - lse[:, None])
    grad = (p - t) / n
    grad[:, Vg:] = 0.0
    if defect == "padding_minus_t":         # (0 - t) * scale written where col >= Vv
        grad[:, Vv:] = -(eps / Vv) / n
    grad = torch.where(counted[:, None], grad, zero)
    if defect == "rows_past_grid_cap_unwritten":
        grad[k.bwd_max_grid_rows:] = 0.0
    xabs = xd[:, :Vv].abs()
    xabs = torch.where(torch.isinf(xabs), torch.zeros_like(xabs), xabs)
    return SimpleNamespace(loss=loss, grad=grad, lse=lse, rowloss=row / n, count=count, n=n,
                           p=p[:, :Vv], t=t[:, :Vv], w=w[:, :Vv], wx=wx, meanx=meanx, counted=counted,
                           xabs=xabs, Vv=Vv, eps=eps, defect=defect)


def scale_grad(ref, gout):
    """The reference gradient for the upstream gradient ``gout`` (the 'gout_dropped' defect uses 1)."""
    return ref.grad * (1.0 if ref.defect == "gout_dropped" else f32(gout))


def top1_ref(x, labels, defect=None):
    """Number of rows whose top-1 index equals the label: NaN above every number, the first
    maximal index (a label that is no column index never hits)."""
    xd = x.double()
    R, V = xd.shape
    nan = torch.isnan(xd)
    if defect == "nan_not_maximal":
        key = torch.where(nan, torch.full_like(xd, -INF), xd)
    else:
        key = torch.where(nan, torch.full_like(xd, INF), xd)
        key = torch.where(nan.any(1, keepdim=True) & ~nan, torch.full_like(xd, -INF), key)
    top = key == key.max(1, keepdim=True).values
    if defect == "last_index_ties":
        arg = V - 1 - (top.flip(1).cumsum(1) == 0).sum(1)
    else:
        arg = (top.cumsum(1) == 0).sum(1)
    return int((arg == labels.long()).sum())


# ------------------------------------------------------------------------------ fp32 model
def _exp32(d):
    return torch.exp2(d * torch.tensor(LOG2E, dtype=torch.float32))


def model32(x, labels, eps, gout, valid_cols=-1, lam=None, fused=False):
    """The kernels' formulas in torch.float32 (sum order aside): the split form (lse kept in
    fp32, p = exp(x - lse)) or the fused form (p = exp(x - max) / sum).  Returns what ``compare``
    takes: loss, grad (x's dtype), count, rowloss, lse."""
    R, V = x.shape
    Vv = classes(V, valid_cols)
    f = torch.float32
    xf = x.float()[:, :Vv]
    e, gs1 = torch.tensor(eps, dtype=f), torch.tensor(gout, dtype=f)
    cols = torch.arange(Vv)
    lab = labels.long()

    def onehot(l):
        return (cols[None, :] == l[:, None]).to(f)

    def logit(l):
        inside = (l >= 0) & (l < Vv)
        return torch.where(inside, xf.gather(1, l.clamp(0, Vv - 1)[:, None])[:, 0],
                           torch.zeros(R, dtype=f))

    m = xf.max(1).values
    se = _exp32(xf - m[:, None]).sum(1)
    lse = m + torch.log(se)
    base_t = e / Vv
    if lam is None:
        counted = lab != IGNORE
        n = max(1, int(counted.sum()))
        xl = logit(lab)
        t = base_t + onehot(lab) * (1 - e)
    else:
        counted = torch.ones(R, dtype=torch.bool)
        n = max(1, R)
        lm = torch.tensor(lam, dtype=f)
        om = 1 - lm
        xl = lm * logit(lab) + om * logit(lab.flip(0))
        t = base_t + (1 - e) * (onehot(lab) * lm + onehot(lab.flip(0)) * om)
    if eps > 0:
        row = (1 - e) * (lse - xl) + e * (lse - xf.sum(1) / Vv)
    else:
        row = lse - xl
    row = torch.where(counted, row, torch.zeros_like(row))
    rowloss = row * (1 / torch.tensor(float(n), dtype=f)) if fused else row / n
    if fused:
        scale = 1 / torch.tensor(float(n), dtype=f)
        p = _exp32(xf - m[:, None]) * (1 / se)[:, None]
    else:
        scale = gs1 / n
        p = _exp32(xf - lse[:, None])
    g = (p - t) * scale * counted[:, None]
    grad = torch.zeros(R, V, dtype=f)
    grad[:, :Vv] = g
    return SimpleNamespace(loss=rowloss.sum(), grad=grad.to(x.dtype), count=int(counted.sum()),
                           rowloss=rowloss, lse=lse)


# ------------------------------------------------------------------------------ comparison
def compare(case, eps, gout, out, ref, dtype):
    """Assert ``out`` (loss, grad, and, where not None, count, rowloss, lse) against the float64
    reference ``ref`` of ``case`` within the bounds of the module docstring; returns the largest
    error / bound ratios {"grad", "grad_p" (elements with p A >= t), "lse",
    "rowloss", "loss"} (0 where nothing was compared).
    Rows with a +inf or NaN class logit, or a -inf one at eps > 0, only have to agree with the
    reference on which outputs are finite."""
    R, V = case.x.shape
    Vv = ref.Vv
    tag = f"{case.name} eps={eps} gout={gout} {DT_ID[dtype]}"
    dev = ref.grad.device
    g = out.grad.detach().to(dev).double()
    g64 = scale_grad(ref, gout)
    assert g.shape == (R, V), tag
    xc = case.x[:, :Vv].to(dev).double()
    mask_only = (torch.isnan(xc) | (xc == INF)).any(1)
    if eps > 0:
        mask_only |= (xc == -INF).any(1)
    full = ~mask_only
    ratios = {"grad": 0.0, "grad_p": 0.0, "lse": 0.0, "rowloss": 0.0, "loss": 0.0}
    # exactly zero: padding columns, ignored rows
    assert not g[:, Vv:].any(), f"{tag}: padding columns are not zero"
    assert not g[~ref.counted].any(), f"{tag}: ignored rows are not zero"
    # which outputs are finite
    fin, fin64 = torch.isfinite(g[:, :Vv]), torch.isfinite(g64[:, :Vv])
    assert torch.equal(fin, fin64), \
        f"{tag}: finite gradient mask differs at {(fin != fin64).nonzero()[:4].tolist()}"
    # per-element gradient bound
    gs = abs(f32(gout)) / ref.n
    A = ref.xabs + ref.lse.abs()[:, None] + 16.0
    bound = gs * (ref.p * A + ref.t) * 2.0 ** -22 + 2.0 ** -60
    if dtype == torch.bfloat16:
        bound = bound + g64[:, :Vv].abs() * 2.0 ** -7
    sel = full[:, None] & ref.counted[:, None] & fin64
    if sel.any():
        err = (g[:, :Vv] - g64[:, :Vv]).abs()
        r = torch.where(sel, err / bound, torch.zeros_like(err))
        ratios["grad"] = r.max().item()
        ratios["grad_p"] = torch.where(ref.p * A >= ref.t, r, torch.zeros_like(r)).max().item()
        if ratios["grad"] > 1.0:
            i, j = divmod(int(r.argmax()), Vv)
            raise AssertionError(f"{tag}: grad[{i},{j}] = {g[i, j].item():.9e}, float64 "
                                 f"{g64[i, j].item():.9e}, |d| = {err[i, j].item():.3e} > bound "
                                 f"{bound[i, j].item():.3e} (ratio {ratios['grad']:.3f})")
        # -inf class columns (eps == 0): exactly zero
        ninf = (xc == -INF) & sel
        assert not g[:, :Vv][ninf].any(), f"{tag}: gradient at a -inf logit is not zero"
        if getattr(case, "ceiling", True):       # the old whole-tensor ceiling (module docstring)
            z = torch.zeros_like(err)
            top, top64 = torch.where(sel, err, z).max().item(), \
                torch.where(sel, g64[:, :Vv].abs(), z).max().item()
            lim = 1e-2 if dtype == torch.bfloat16 else 1e-5
            assert top <= lim * top64, f"{tag}: whole-tensor {top:.3e} / {top64:.3e} > {lim}"
    if out.count is not None:
        assert int(out.count) == ref.count, f"{tag}: count {int(out.count)} != {ref.count}"
    if out.lse is not None:
        l, l64 = out.lse.detach().to(dev).double(), ref.lse
        assert torch.equal(torch.isfinite(l), torch.isfinite(l64)), f"{tag}: finite lse mask"
        okr = torch.isfinite(l64)
        if okr.any():
            lb = (l64.abs() + ref.xabs.max(1).values + 16.0) * 2.0 ** -22
            r = torch.where(okr, (l - l64).abs() / lb, torch.zeros_like(lb))
            ratios["lse"] = r.max().item()
            assert ratios["lse"] <= 1.0, \
                f"{tag}: lse[{int(r.argmax())}] off by {ratios['lse']:.3f} of its bound"
    rb = (ref.lse.abs() + ref.wx.abs() + (ref.meanx.abs() if eps > 0 else 0.0) + 16.0) \
        * 2.0 ** -21 / ref.n
    if out.rowloss is not None:
        rl, rl64 = out.rowloss.detach().to(dev).double(), ref.rowloss
        assert torch.equal(torch.isfinite(rl), torch.isfinite(rl64)), f"{tag}: finite row losses"
        assert not rl[~ref.counted].any(), f"{tag}: row loss of an ignored row is not zero"
        okr = torch.isfinite(rl64) & ref.counted
        if okr.any():
            r = torch.where(okr, (rl - rl64).abs() / rb, torch.zeros_like(rb))
            ratios["rowloss"] = r.max().item()
            assert ratios["rowloss"] <= 1.0, \
                f"{tag}: row loss [{int(r.argmax())}] off by {ratios['rowloss']:.3f} of its bound"
    loss, loss64 = float(out.loss), float(ref.loss)
    assert math.isfinite(loss) == math.isfinite(loss64), f"{tag}: loss {loss} vs {loss64}"
    if math.isfinite(loss64):
        if ref.count == 0 and case.lam is None:
            assert loss == 0.0, f"{tag}: no counted row, loss {loss}"
        lbound = float(rb[ref.counted].sum()) + abs(loss64) * 2.0 ** -20
        ratios["loss"] = abs(loss - loss64) / lbound if lbound > 0 else 0.0
        assert ratios["loss"] <= 1.0, \
            f"{tag}: loss {loss!r} vs float64 {loss64!r}: {ratios['loss']:.3f} of its bound"
        c = ref.counted
        if c.any() and abs(loss64) >= 2.0 ** -6 * float((ref.lse.abs() + ref.wx.abs())[c].mean()):
            assert abs(loss - loss64) <= 1e-4 * abs(loss64), f"{tag}: loss {loss} vs {loss64}"
    return ratios


# ------------------------------------------------------------------------------ case builders
def _case(name, x, labels, valid_cols=-1, lam=None, dtype=torch.float32, ceiling=True):
    """``ceiling``: the case also meets the old whole-tensor gradient limit (module docstring)."""
    return SimpleNamespace(name=name, x=x.to(dtype), labels=labels.long(), valid_cols=valid_cols,
                           lam=lam, ceiling=ceiling)


def _random(name, R, V, valid_cols, dtype, lam=None, scale=3.0, ignore=(), seed=0, ceiling=True):
    Vv = classes(V, valid_cols)
    g = torch.Generator().manual_seed(1000003 * R + 101 * V + 7 * Vv + seed)
    x = torch.randn(R, V, generator=g) * scale
    labels = torch.randint(0, Vv, (R,), generator=g)
    for r in ignore:
        labels[r] = IGNORE
    return _case(name, x, labels, valid_cols, lam, dtype, ceiling)


def vector_valid_cols(V, k=CPU_CONSTS):
    """valid_cols of the vector path at V: all; inside the last vector; one vector short; one
    past the first vector; 5 at one item per thread (most lanes and three waves empty); 1."""
    vs = [V, V - 1, V - (k.vec - 1), V - k.vec, k.vec + 1, 1]
    if V == k.threads * k.vec:
        vs.append(5)
    return sorted({v for v in vs if 1 <= v <= V}, reverse=True)


@functools.lru_cache(maxsize=None)
def column_cases_vector(dtype, k_threads=256, k_vec=8):
    """R = 5, one ignored row (hard); V: one item, one short of / exactly / one past one item per
    thread (the last: a second forward trip and a second ce_bwd column block with one live
    thread), and two full trips + 1."""
    item = k_threads * k_vec
    out = []
    for V in (k_vec, item - k_vec, item, item + k_vec, 2 * item + k_vec):
        assert V % k_vec == 0
        for vc in vector_valid_cols(V, SimpleNamespace(threads=k_threads, vec=k_vec)):
            for lam in (None, 0.3):
                out.append(_random(f"vec V={V} Vv={vc} {'hard' if lam is None else 'pair'}", 5, V,
                                   vc, dtype, lam, ignore=(1,) if lam is None else ()))
    return out


@functools.lru_cache(maxsize=None)
def column_cases_scalar(dtype, k_threads=256, k_vec=8):
    out = []
    for V in (1, 7, k_threads - 1, k_threads, k_threads + 1, 2 * k_threads + 1, 1001):
        assert V % k_vec != 0 or V == k_threads   # V = threads runs the vector path: kept as listed
        for vc in sorted({V, max(1, V - 1), 1}, reverse=True):
            for lam in (None, 0.3):
                out.append(_random(f"scalar V={V} Vv={vc} {'hard' if lam is None else 'pair'}", 5,
                                   V, vc, dtype, lam, ignore=(3,) if lam is None else ()))
    return out


IGNORE_PATTERNS = ("none", "one", "every_second", "all", "only_last_valid")


@functools.lru_cache(maxsize=None)
def row_cases(dtype, k_threads=256):
    """The one-block strided loops of ce_count_kernel / ce_sum_kernel: R around one and two trips."""
    out = []
    for R in (1, 2, 3, k_threads - 1, k_threads, k_threads + 1, 2 * k_threads + 1):
        for pat in IGNORE_PATTERNS:
            ign = {"none": [], "one": [R // 2], "every_second": list(range(0, R, 2)),
                   "all": list(range(R)), "only_last_valid": list(range(R - 1))}[pat]
            out.append(_random(f"rows R={R} ignore={pat}", R, 16, -1, dtype, None, ignore=ign))
    return out


@functools.lru_cache(maxsize=None)
def grid_row_cases(dtype, cap=65535, k_vec=8):
    """ce_bwd's grid.y cap: R = cap (one trip), +1 and +2 (a second trip of one / two rows),
    2 cap + 1 (one row in the third trip); vector (V = 8) and scalar (V = 7)."""
    out = []
    for R in (cap, cap + 1, cap + 2, 2 * cap + 1):
        for V in (k_vec, k_vec - 1):
            out.append(_random(f"grid R={R} V={V} hard", R, V, -1, dtype, None,
                               ignore=range(5, R, 97)))
            out.append(_random(f"grid R={R} V={V} pair", R, V, -1, dtype, 0.3))
    return out


def out_of_range_labels(V, Vv):
    return (-1, Vv, V, V + 5)


@functools.lru_cache(maxsize=None)
def label_cases(dtype):
    """Labels outside [0, Vv) on rows that are not the last and on the last, hard and pair."""
    out = []
    for V, vc in ((8, -1), (16, 11), (7, -1), (13, 9), (2056, 2050)):
        Vv = classes(V, vc)
        oor = out_of_range_labels(V, Vv)
        for last in oor:
            for lam in (None, 0.3):
                c = _random(f"labels V={V} Vv={Vv} last={last} {'hard' if lam is None else 'pair'}",
                            8, V, vc, dtype, lam)
                c.labels[:4] = torch.tensor(oor)
                c.labels[5] = IGNORE if lam is None else 1
                c.labels[7] = last
                out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def pair_cases(dtype):
    """lam x R (odd R: the middle row is its own partner), rows with a == b, labels outside."""
    out = []
    for V, vc in ((40, -1), (37, 33)):
        Vv = classes(V, vc)
        for R in (1, 2, 3, 256, 257):
            for lam in (0.0, 1.0, 0.5, 0.3):
                c = _random(f"pair V={V} Vv={Vv} R={R} lam={lam}", R, V, vc, dtype, lam)
                if R >= 2:
                    c.labels[R - 1] = c.labels[0]           # a == b on the first and last row
                if R >= 256:
                    c.labels[10], c.labels[20], c.labels[R - 31] = -1, Vv, V + 5
                out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def magnitude_cases(dtype):
    out = []
    for V in (1000, 257):
        g = torch.Generator().manual_seed(V)
        R = 16
        lab = torch.randint(0, V, (R,), generator=g)
        out.append(_random(f"mag V={V} randn*30", R, V, -1, dtype, scale=30.0, ceiling=False))
        out.append(_random(f"mag V={V} randn*100", R, V, -1, dtype, scale=100.0, ceiling=False))
        out.append(_random(f"mag V={V} randn*100 pair", R, V, -1, dtype, 0.3, scale=100.0,
                           ceiling=False))
        x = torch.zeros(R, V)
        x[torch.arange(R), (lab + torch.arange(R) % 2) % V] = 80.0   # on the label / next to it
        out.append(_case(f"mag V={V} dominant +80", x, lab, dtype=dtype, ceiling=False))
        x = torch.zeros(R, V)
        x[torch.arange(R), (lab + torch.arange(R) % 2) % V] = -80.0
        out.append(_case(f"mag V={V} one -80", x, lab, dtype=dtype, ceiling=False))
        for cval in (0.0, 7.5, -1e4):
            out.append(_case(f"mag V={V} constant {cval}", torch.full((R, V), cval), lab,
                             dtype=dtype, ceiling=abs(cval) < 30))
        x = torch.randint(-64, 65, (R, V), generator=g).float() / 8     # exact in bf16
        assert torch.equal(x.bfloat16().float(), x)
        out.append(_case(f"mag V={V} bf16-exact", x, lab, dtype=dtype))
    return out


@functools.lru_cache(maxsize=None)
def exact_cases(dtype):
    """Constant rows, Vv and n powers of two: with eps = 0 and gout = 1 the fused form's gradient
    is exactly (1/Vv - [c == label]) / n (Vv <= 128 for bf16: (Vv-1)/Vv needs log2 Vv + 1 bits)."""
    out = []
    shapes = [(8, -1), (64, -1), (136, 128), (67, 64), (16, 8)]
    if dtype == torch.float32:
        shapes += [(2048, -1), (4104, 4096), (1001, 512)]
    for V, vc in shapes:
        Vv = classes(V, vc)
        for R, ign in ((4, ()), (5, (2,)), (1, ())):
            for cval in (0.0, 7.5):
                lab = (torch.arange(R) * 3 + 1) % Vv
                for r in ign:
                    lab[r] = IGNORE
                out.append(_case(f"exact V={V} Vv={Vv} R={R} c={cval}", torch.full((R, V), cval),
                                 lab, vc, dtype=dtype))
    return out


def exact_grad(case):
    """The exact fused gradient of an exact case (float64)."""
    R, V = case.x.shape
    Vv = classes(V, case.valid_cols)
    counted = case.labels != IGNORE
    n = max(1, int(counted.sum()))
    g = torch.zeros(R, V, dtype=torch.float64)
    g[:, :Vv] = 1.0 / Vv
    rows = torch.arange(R)[counted]
    g[rows, case.labels[counted]] -= 1.0
    g[~counted] = 0.0
    return g / n


@functools.lru_cache(maxsize=None)
def nonfinite_cases(dtype):
    """-inf in non-label class columns (within the bounds at eps = 0: a finite loss, gradient 0
    there); +inf / NaN rows (agreement on what is finite); NaN / inf in padding columns (no
    effect at all).  A NaN stands in the first and in a later column of a thread of the scalar
    forward, and alone in a 16-byte item of the vector forward."""
    out = []
    for V, vc in ((16, -1), (13, -1), (24, 19), (2056, 2050), (513, -1)):
        Vv = classes(V, vc)
        for lam in (None, 0.3):
            form = "hard" if lam is None else "pair"
            c = _random(f"nonfinite V={V} Vv={Vv} -inf {form}", 6, V, vc, dtype, lam)
            c.labels[:] = torch.tensor([0, 1, 2, 3, 2, 1])         # columns 0..3 hold labels
            x = c.x.float()
            x[0, 4] = -INF
            x[1, 5:Vv] = -INF                                       # whole lanes / waves of -inf
            x[2, Vv - 1] = -INF
            x[4, 4:Vv:2] = -INF
            c.x = x.to(dtype)
            out.append(c)
            c = _random(f"nonfinite V={V} Vv={Vv} nan/+inf {form}", 6, V, vc, dtype, lam)
            c.labels[:] = torch.tensor([0, 1, 2, 3, 2, 1])
            x = c.x.float()
            x[0, 4] = NAN
            x[1, Vv - 1] = INF
            x[2, 0] = NAN
            x[2, Vv // 2] = NAN
            x[4, 5] = INF
            x[4, 6] = -INF
            c.x = x.to(dtype)
            out.append(c)
            if Vv < V:
                c = _random(f"nonfinite V={V} Vv={Vv} padding {form}", 6, V, vc, dtype, lam)
                x = c.x.float()
                x[0, Vv] = NAN
                x[1, V - 1] = INF
                x[2, Vv:] = -INF
                x[3, Vv] = 1e30
                c.x = x.to(dtype)
                out.append(c)
    return out


def all_cases(dtype, big=True):
    cs = (column_cases_vector(dtype) + column_cases_scalar(dtype) + row_cases(dtype)
          + label_cases(dtype) + pair_cases(dtype) + magnitude_cases(dtype) + exact_cases(dtype)
          + nonfinite_cases(dtype))
    return cs + grid_row_cases(dtype) if big else cs


# ------------------------------------------------------------------------------ top-1 cases
TOP1_R = (1, 3, 4, 5, 1021)
TOP1_V = (1, 2, 63, 64, 65, 129, 1000)


def top1_special_rows(V):
    """[(row fp32 [V], label)] with values exact in bf16; which rows exist depends on V."""
    def row(fill=-2.0, **at):
        x = torch.full((V,), fill)
        for c, v in at.items():
            x[int(c[1:]) % V] = v
        return x
    last = V - 1
    rows = [
        (row(c0=5.0), 0),                                   # the maximum in column 0
        (row(**{f"c{last}": 5.0}), last),                   # ... in the last column
        (torch.full((V,), 0.5), 0),                         # all equal: the first wins
        (torch.full((V,), 0.5), last),                      # ... and the last does not (V > 1)
        (torch.full((V,), -INF), 0),                        # all -inf: index 0
        (torch.full((V,), -INF), min(1, last)),             # ... label 1 misses (V > 1)
        (row(c0=NAN), 0),                                   # NaN first
        (row(**{f"c{last}": NAN, "c0": 9.0}), last),        # NaN last beats a number
        (row(c0=3.0), IGNORE),                              # labels that are no index: never a hit
        (row(c0=3.0), V),
        (row(**{f"c{last}": INF, "c0": INF}), 0),           # +inf tie: the first
        (row(**{f"c{last}": INF, "c0": INF}), last),
    ]
    if V >= 2:
        rows += [(row(c0=4.0, c1=4.0), 0), (row(c0=4.0, c1=4.0), 1)]      # tie across lanes
        rows += [(row(**{"c0": NAN, f"c{last}": NAN}), 0),                # two NaNs: the first
                 (row(**{"c0": NAN, f"c{last}": NAN}), last)]
        rows += [(row(c0=7.0, c1=NAN), 1), (row(c0=7.0, c1=NAN), 0)]
        rows += [(row(c0=-INF, c1=-INF, fill=-INF), 1)]
    if V > 64:                                               # tie within one lane's columns
        rows += [(row(c0=4.0, c64=4.0), 0), (row(c0=4.0, c64=4.0), 64),
                 (row(c1=6.0, c64=6.0), 1), (row(c1=6.0, c64=6.0), 64)]
    return rows


@functools.lru_cache(maxsize=None)
def top1_case(dtype, R, V, start=0):
    """Random rows (a third of them hits) with the special rows written from ``start`` on into
    rows 0.., as many as fit."""
    g = torch.Generator().manual_seed(31 * R + V)
    x = torch.randn(R, V, generator=g) * 3
    labels = torch.randint(0, V, (R,), generator=g)
    labels[::3] = x.to(dtype)[::3].float().argmax(1)
    sp = top1_special_rows(V)
    for i, (xr, y) in enumerate(sp[start:start + R]):
        x[i] = xr
        labels[i] = y
    return x.to(dtype), labels


def top1_starts(R, V):
    return range(0, len(top1_special_rows(V)), R)
