"""Inputs and float64 references shared by the eval_stats tests (CPU and GPU).

``special_rows`` holds the hand-written cases of the kernel's contract: every row comes with the
expectation worked out by hand from the rules in ``mipipe.ops._ref.eval_stats``'s docstring.
"""
import functools

import torch

IGNORE = -100
INF = float("inf")
NAN = float("nan")


def _row(V, head, fill=-2.0):
    x = torch.full((V,), fill, dtype=torch.float32)
    x[:len(head)] = torch.tensor(head, dtype=torch.float32)
    return x


def special_rows(V, Vv):
    """[(logits row fp32 [V] (values exact in bf16), label, expectation)], V >= Vv >= 10.
    The expectation is "skip", "invalid" or (pred, rank, loss is finite)."""
    rows = [
        # duplicates of the label's value below (column 0) and above (column 4) the label:
        # greater 3 and 5, equal-and-below one -> rank 3
        (_row(V, [1, 3, 1, 5, 1, 0]), 2, (3, 3, True)),
        # a tie at the maximum: the first index wins; the last of the three has rank 2
        (_row(V, [0, 4, 4, 1, 4]), 4, (1, 2, True)),
        (_row(V, [0, 4, 4, 1, 4]), 1, (1, 0, True)),
        # an all-equal row: pred 0, the label's rank is its index
        (torch.full((V,), 0.5), 3, (0, 3, True)),
        # -inf entries; with the label on one of them every number is greater: loss +inf
        (_row(V, [-INF, 2, -INF, 1]), 3, (1, 1, True)),
        (_row(V, [-INF, 2, -INF, 1]), 0, (1, Vv - 2, False)),
        # an all -inf row: everything is equal, lse = -inf, loss = nan
        (torch.full((V,), -INF), 2, (0, 2, False)),
        # NaN rows: NaN is the maximum, NaNs are equal to each other
        (_row(V, [1, NAN, 7, NAN]), 2, (1, 2, False)),
        (_row(V, [1, NAN, 7, NAN]), 3, (1, 1, False)),
        (_row(V, [1, NAN, 7, NAN]), 1, (1, 0, False)),
        # +inf rows: loss is inf - inf or inf
        (_row(V, [0, INF, 2]), 1, (1, 0, False)),
        (_row(V, [0, INF, 2]), 2, (1, 1, False)),
        # ignored rows are counted nowhere (their logits may be anything)
        (_row(V, [NAN, 1, 2]), IGNORE, "skip"),
        (_row(V, [3, 1, 2]), IGNORE, "skip"),
        # invalid labels
        (_row(V, [3, 1, 2]), -1, "invalid"),
        (_row(V, [3, 1, 2]), Vv, "invalid"),
        (_row(V, [3, 1, 2]), V, "invalid"),
        (_row(V, [3, 1, 2]), 1 << 40, "invalid"),
    ]
    # the largest value (and a NaN) in padded columns when there are any: they enter nothing
    x = _row(V, [0, 2, 1])
    if Vv < V:
        x[Vv] = 100.0
        x[V - 1] = NAN
    rows.append((x, 1, (1, 0, True)))
    # one clear winner over an otherwise equal row: a hit with a low confidence,
    # e^6 / (e^6 + Vv - 1).  At Vv = 30522 that is 0.013: it shares the lowest of 64 bins with the
    # all-equal row, whose confidence 1 / 30522 = 549.7 * 2^-24 alone could not be held in Q24 to
    # 1e-4 relative (rounding to 550 is 6e-4 off; the pair's sum is 5e-6 off)
    rows.append((_row(V, [6.5], fill=0.5), 0, (0, 0, True)))
    return rows


@functools.lru_cache(maxsize=None)
def make_inputs(dtype, R, V, valid_cols, seed=0):
    """(logits [R, V] of ``dtype``, labels int64 [R]) on the CPU: random logits x 3 with the special
    rows written into rows 0 .. (as many as fit).  Cached: treat as read-only."""
    Vv = valid_cols if 0 < valid_cols < V else V
    g = torch.Generator().manual_seed(1000 * seed + R + V)
    logits = (torch.randn(R, V, generator=g) * 3).to(dtype)
    labels = torch.randint(0, Vv, (R,), generator=g)
    labels[::5] = logits[::5, :Vv].float().argmax(1)  # a fifth of the rows are hits
    for i, (x, y, _) in enumerate(special_rows(V, Vv)[:R]):
        logits[i] = x.to(dtype)
        labels[i] = y
    return logits, labels


def f64_stats(logits, labels, valid_cols, bins):
    """Float64 per-row quantities of the counted rows: dict of ``ok`` (row mask: label valid and
    not ignored), ``loss`` and ``conf`` (float64 [R], nan where not ok) and ``finite`` (loss finite)."""
    R, V = logits.shape
    Vv = valid_cols if 0 < valid_cols < V else V
    ok = (labels != IGNORE) & (labels >= 0) & (labels < Vv)
    x = logits[:, :Vv].double()
    lse = torch.logsumexp(x, 1)
    xy = x.gather(1, labels.clamp(0, Vv - 1)[:, None])[:, 0]
    loss = torch.where(ok, lse - xy, torch.full_like(lse, NAN))
    nan_row = (x != x).any(1)
    mx = torch.where(x != x, torch.full_like(x, -INF), x).max(1).values
    conf = torch.where(ok & ~nan_row, torch.exp(mx - lse), torch.full_like(lse, NAN))
    return {"ok": ok, "loss": loss, "conf": conf, "finite": ok & torch.isfinite(loss)}


def near_bin_edge(conf64, bins, margin=1e-3):
    """Rows whose float64 ``conf * bins`` lies within ``margin`` of an integer that separates two
    bins (1 .. bins-1): an fp32 confidence (at most 4.3e-5 bin units away) could fall into the
    neighbouring bin.  0 and ``bins`` separate nothing: a confidence is never negative and the top
    bin is clamped, so a row next to them (an all-equal row of a 30,522-class vocabulary has
    ``conf * bins`` = 5e-4) stays in its bin and stays in the test."""
    t = conf64 * bins
    edge = torch.round(t)
    return torch.isfinite(t) & ((t - edge).abs() < margin) & (edge >= 1) & (edge <= bins - 1)
