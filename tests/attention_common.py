"""Shared by the attention reference tests (CPU) and the attention sweep (GPU): an independent
float64 reference of the packed-layout attention forward + backward, a bf16 model of the kernel
design's unavoidable roundings, the input cases, and the per-slice error measure.

Layout as in attention.hip: qkv [B*S, 3*H*64] (q | k | v, head-major), o / do [B*S, H*64],
lse [B, H, S] (natural log), mask [B, S] additive key bias, dqkv like qkv."""
import functools
import math

import torch

D = 64
SCALE = 1.0 / math.sqrt(D)
NEG = -10000.0

O_TOL = 2e-2      # the project's attention tolerances, applied per (batch, head) slice
DQKV_TOL = 3e-2
FLOOR_FRAC = 0.25

# lse: |lse - ref| <= LSE_TOL * max(1, |ref|).  LSE_FP32_ERR is the largest such relative error of
# an fp32 evaluation of the reference (lse_fp32 below) against float64 over every sweep input,
# measured by test_attention_ref_cpu.py::test_lse_fp32_error_sets_tolerance: 4.14e-7 (B=2, S=65,
# H=2, lead mask: one kept key, lse is a single 64-term fp32 dot product), rounded up to 5e-7.
# The factor 16 covers base-2 hardware exp / log and another fp32 summation order:
# LSE_TOL = 16 * 5e-7 = 8e-6.
LSE_FP32_ERR = 5e-7
LSE_TOL = 16 * LSE_FP32_ERR

MASK_KINDS = ("none", "ragged", "lead", "ragged_inf", "lead_inf")


def bf16r(t):
    """Round to bf16, keep float64."""
    return t.to(torch.bfloat16).double()


def _split(qkv, B, S, H):
    x = qkv.double().reshape(B, S, 3, H, D)
    return tuple(x[:, :, i].transpose(1, 2) for i in range(3))  # [B, H, S, D]


def _rows(t):
    """[B, H, S, D] -> [B*S, H*D]"""
    B, H, S, _ = t.shape
    return t.transpose(1, 2).reshape(B * S, H * D)


def _softmax(s):
    """(p, lse) of the last axis; -inf entries give exact zeros, a row of only -inf gives
    p = 0 and lse = -inf, never NaN."""
    m = s.max(-1, keepdim=True).values
    mu = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - mu)
    l = e.sum(-1, keepdim=True)
    ok = l > 0
    ls = torch.where(ok, l, torch.ones_like(l))
    p = torch.where(ok, e / ls, torch.zeros_like(e))
    lse = torch.where(ok, mu + torch.log(ls), torch.full_like(l, -math.inf))
    return p, lse.squeeze(-1)


def _attention(qkv, do, B, S, H, mask, scale, keep, p_drop, rnd):
    q, k, v = _split(qkv, B, S, H)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if mask is not None:
        s = s + mask.double().reshape(B, 1, 1, S)
    p, lse = _softmax(s)
    kp = None if keep is None else keep.double() / (1.0 - p_drop)
    pd = p if kp is None else p * kp
    o = rnd(torch.einsum("bhqk,bhkd->bhqd", rnd(pd), v))
    dof = do.double().reshape(B, S, H, D).transpose(1, 2)
    dv = torch.einsum("bhqk,bhqd->bhkd", rnd(pd), dof)
    dp = torch.einsum("bhqd,bhkd->bhqk", dof, v)
    if kp is not None:
        dp = dp * kp
    delta = (dof * o).sum(-1, keepdim=True)
    ds = rnd(p * (dp - delta) * scale)
    dq = torch.einsum("bhqk,bhkd->bhqd", ds, k)
    dk = torch.einsum("bhqk,bhqd->bhkd", ds, q)
    dqkv = torch.cat([_rows(dq), _rows(dk), _rows(dv)], 1)
    return _rows(o), lse, rnd(dqkv)


def attention_f64(qkv, do, B, S, H, mask, scale, keep=None, p_drop=0.0):
    """(o [B*S, H*D], lse [B, H, S], dqkv [B*S, 3*H*D]) in float64 from the bf16-rounded inputs
    alone: closed-form backward with delta = sum_d dO*O of its own float64 O.  ``keep`` is
    ``_ref.attention_keep(B, S, H, p_drop, seed, ...)`` for attention-probability dropout."""
    return _attention(qkv, do, B, S, H, mask, scale, keep, p_drop, lambda t: t)


def attention_bf16_model(qkv, do, B, S, H, mask, scale, keep=None, p_drop=0.0):
    """The same math with the roundings no bf16 flash kernel avoids: P and dS to bf16 before
    their second matmul, O (which then feeds delta) and dQKV to bf16.  A model of the design,
    not of the code: it only shows that the tolerances are attainable."""
    return _attention(qkv, do, B, S, H, mask, scale, keep, p_drop, bf16r)


def lse_fp32(qkv, B, S, H, mask, scale):
    """The reference's lse evaluated in fp32 (what sets the lse tolerance)."""
    x = qkv.float().reshape(B, S, 3, H, D)
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if mask is not None:
        s = s + mask.float().reshape(B, 1, 1, S)
    return _softmax(s)[1]


def kept_keys(B, S, mask_kind):
    """[B, S] bool: the keys a mask kind keeps."""
    kind = mask_kind.replace("_inf", "")
    keep = torch.ones(B, S, dtype=torch.bool)
    if kind == "ragged":
        for b in range(B):
            keep[b, max(1, S * (b + 1) // (B + 1)):] = False
    elif kind == "lead":
        keep[:, :min(70, S - 1)] = False
    else:
        assert kind == "none", mask_kind
    return keep


def make_mask(B, S, mask_kind):
    assert mask_kind in MASK_KINDS, mask_kind
    if mask_kind == "none":
        return None
    mask = torch.zeros(B, S)
    mask[~kept_keys(B, S, mask_kind)] = -math.inf if mask_kind.endswith("_inf") else NEG
    return mask


def make_case(B, S, H, mask_kind, seed):
    """(qkv bf16, do bf16, mask fp32 or None) on the CPU; the data do not depend on the mask."""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * S, 3 * H * D, generator=g) * 1.5).to(torch.bfloat16)
    do = torch.randn(B * S, H * D, generator=g).to(torch.bfloat16)
    return qkv, do, make_mask(B, S, mask_kind)


def case_seed(B, S, H):
    return 1000 * S + 10 * H + B


@functools.lru_cache(maxsize=None)
def case_and_reference(B, S, H, mask_kind):
    """make_case and its float64 reference, computed once per process; treat as read-only."""
    qkv, do, mask = make_case(B, S, H, mask_kind, case_seed(B, S, H))
    return qkv, do, mask, attention_f64(qkv, do, B, S, H, mask, SCALE)


def sweep_cases():
    """(B, S, H, mask_kind) of the GPU tolerance sweep."""
    cases = [(2, 1, 3, "none")]
    for S in (31, 33, 63, 65, 127, 129, 193, 257):
        cases += [(2, S, 3, mk) for mk in ("none", "ragged", "lead")]
    cases += [(1, 2048, 2, mk) for mk in ("none", "ragged", "lead")]
    cases += [(2, S, 12, "none") for S in (33, 129)]
    return cases


def inf_cases():
    """-inf masks that leave every sample at least one key (exact-zero gradient checks)."""
    return [(2, S, 2, mk) for S in (65, 129, 257)
            for mk in ("ragged", "lead", "ragged_inf", "lead_inf")]


def slice_err(a, ref, floor):
    """a, ref [B, S, H, D]-shaped views of one of O / dQ / dK / dV.  Per (batch, head) slice:
    max |a - ref| / max(max |ref| of the slice, floor).  Returns (worst error, (b, h))."""
    a, ref = a.double(), ref.double()
    err = (a - ref).abs().amax(dim=(1, 3))
    den = ref.abs().amax(dim=(1, 3)).clamp_min(floor)
    e = err / den
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)  # NaN never passes
    i = int(e.argmax())
    return float(e.flatten()[i]), (i // e.shape[1], i % e.shape[1])


def tensor_errors(o, dqkv, ref_o, ref_dqkv, B, S, H):
    """{name: (worst slice error, (b, h))} for O, dQ, dK, dV with the 25 % floors: of the largest
    |ref| of O for O, of the whole dQKV for the three gradients."""
    out = {}
    if o is not None:
        floor = FLOOR_FRAC * float(ref_o.abs().max())
        out["O"] = slice_err(o.reshape(B, S, H, D), ref_o.reshape(B, S, H, D), floor)
    if dqkv is not None:
        floor = FLOOR_FRAC * float(ref_dqkv.abs().max())
        a, r = dqkv.reshape(B, S, 3, H, D), ref_dqkv.reshape(B, S, 3, H, D)
        for i, name in enumerate(("dQ", "dK", "dV")):
            out[name] = slice_err(a[:, :, i], r[:, :, i], floor)
    return out


def lse_err(lse, ref):
    """max |lse - ref| / max(1, |ref|); matching infinities count as exact."""
    lse, ref = lse.double(), ref.double()
    same_inf = torch.isinf(ref) & (lse == ref)
    e = (lse - ref).abs() / ref.abs().clamp_min(1.0)
    e = torch.where(same_inf, torch.zeros_like(e), e)
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    return float(e.max())


def assert_close_to_reference(o, lse, dqkv, ref, B, S, H, frac=1.0, what=""):
    """The sweep's tolerance assertions; ``frac`` scales the O / dQKV tolerances (the
    attainability test passes 0.5).  Prints every figure, names the worst slice on failure."""
    ref_o, ref_lse, ref_dqkv = ref
    errs = tensor_errors(o, dqkv, ref_o, ref_dqkv, B, S, H)
    le = None if lse is None else lse_err(lse, ref_lse)
    print(f"{what} B={B} S={S} H={H}: " + " ".join(
        f"{n}={e:.2e}@b{b}h{h}" for n, (e, (b, h)) in errs.items())
        + ("" if le is None else f" lse={le:.2e}"))
    bad = [f"{n}: {e:.3e} at (batch {b}, head {h}) >= {frac * (O_TOL if n == 'O' else DQKV_TOL):.1e}"
           for n, (e, (b, h)) in errs.items()
           if not e < frac * (O_TOL if n == "O" else DQKV_TOL)]
    if le is not None and not le <= LSE_TOL:
        bad.append(f"lse: {le:.3e} > {LSE_TOL:.2e}")
    assert not bad, f"{what} B={B} S={S} H={H}: " + "; ".join(bad)
