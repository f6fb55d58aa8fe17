"""Shared by the BatchNorm edge tests (CPU: test_bn_edges_cpu.py, GPU: test_bn_edges_gpu.py): a
Python mirror of bn.hip's launch geometry, the input constructions, float64 references of the four
training passes (with switchable defects, the "mutants"), fp32 models of the kernels' arithmetic
and the error bounds.

Geometry (csrc/kernels/bn.hip, constants in launchers.hpp): blocks of ``threads`` threads; a thread
owns one 8-channel group, ``tpr = C/8`` threads cover a row and ``rpb = threads // tpr`` rows are
walked per block pass (``C/8 > threads``: ``tpr = threads``, ``rpb = 1`` and several channel passes).
The apply passes give every block a tile of ``rpb * U`` rows; the reduction runs
``bn_bwd_reduce_blocks`` blocks, each thread taking ``row_u`` rows per trip at stride ``G * rpb``.

Exact cases.  Inputs are small integers and per-channel coefficients are signed powers of two (or
quarters), so every product, every partial sum in any order and every result is an exact fp32
number (and an exact bf16 number where bf16 is stored): the comparison with float64 is
``torch.equal`` and a missing term, row or channel moves the result by whole steps.
``assert_exact`` states the condition.

Random cases.  Per element ``|out - ref| <= 2^-8 |ref| + 16 * 2^-24 * T`` for bf16 outputs and the
second term alone for fp32: ``T`` is the sum of the magnitudes of the terms of the expression as
the kernel writes it; ``2^-8`` of the value is the most that rounding to bf16 (8 significant bits)
moves it; and 16 fp32 half-ulps of ``T`` cover the at most about ten roundings of the coefficient
chain and the sum (and what they add to the value that is then rounded to bf16).
Reductions, per channel: ``(chain + 3) * 2^-24 * sum|terms|`` where ``chain`` is the longest
sequence of additions a value passes through (``reduce_chain``) and 3 the roundings of one term.
"""
import functools
import zlib
from types import SimpleNamespace

import torch

U24 = 2.0 ** -24          # fp32 round-to-nearest half-ulp
EXACT = 2 ** 24
EPS = 1e-5

# The launch constants of launchers.hpp as this file was written.  Only the CPU test uses them (it
# has no extension to ask); the GPU test reads the exported values and passes its own namespace.
CPU_CONSTS = SimpleNamespace(threads=256, row_u=4, apply_u=2, reduce_blocks=1024,
                             atomic_budget=1 << 20, min_blocks=64, row_iters=16,
                             det_chunk_rows=64, replicas=16)

C_LIST = [8, 40, 64, 1000, 2048, 2056, 4096]
DT_ID = {torch.bfloat16: "bf16", torch.float32: "fp32"}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------ launch geometry
def row_map(C, k):
    """(tpr, rpb, passes) of bn.hip's row_map."""
    chunks = C // 8
    if chunks <= k.threads:
        return chunks, k.threads // chunks, 1
    return k.threads, 1, cdiv(chunks, k.threads)


def reduce_blocks(M, C, k):
    """bn_bwd_reduce_blocks; also which limit binds: 'rows' | 'budget' | 'floor' | 'cap'."""
    _, rpb, _ = row_map(C, k)
    budget = k.atomic_budget // (3 * C)
    cap = max(k.min_blocks, budget)
    want = cdiv(M, rpb * k.row_iters)
    G = max(1, min(k.reduce_blocks, cap, want))
    if G == want or want < 1:
        why = "rows"
    elif k.reduce_blocks <= cap:
        why = "cap"
    else:
        why = "floor" if budget < k.min_blocks else "budget"
    return G, why


def apply_grid(M, C, u, k):
    _, rpb, _ = row_map(C, k)
    return max(1, cdiv(M, rpb * u))


def apply_rows(C, u, k):
    """The M values of the apply passes for one C, each with the edge it crosses asserted:
    one row; less than one block pass; exactly one tile; one row into the second block (its other
    U*rpb - 1 row slots clamp to M-1 and break); a last tile one row short."""
    _, rpb, _ = row_map(C, k)
    tile = rpb * u
    out = {}
    out["one"] = 1
    out["sub_pass"] = max(1, rpb - 1)
    out["tile"] = tile
    out["tile_plus_1"] = tile + 1
    out["three_tiles_minus_1"] = 3 * tile - 1
    assert apply_grid(out["one"], C, u, k) == 1 and apply_grid(out["sub_pass"], C, u, k) == 1
    assert out["sub_pass"] < rpb or rpb == 1
    assert apply_grid(tile, C, u, k) == 1 and apply_grid(tile + 1, C, u, k) == 2
    assert apply_grid(3 * tile - 1, C, u, k) == 3 and (3 * tile - 1) % tile == tile - 1
    return out


def last_trip_rows(M, C, k):
    """The set of row counts (1..row_u) that the LAST trip of some thread of bn_bwd_reduce_kernel
    holds (threads with no row at all are left out)."""
    _, rpb, _ = row_map(C, k)
    G, _ = reduce_blocks(M, C, k)
    stride = G * rpb
    seen = set()
    for first in range(min(stride, M)):       # one thread per (block, row group)
        n = cdiv(M - first, stride)           # rows this thread owns
        seen.add((n - 1) % k.row_u + 1)
    return seen


def reduce_rows(C, k):
    """The M values of the reduction's tail cases for one C (all on a single block, so the stride
    is rpb): one row; less than a block pass; one short of and one past a full row_u trip; second
    trips of 1, 2 and 3 rows."""
    _, rpb, _ = row_map(C, k)
    u = k.row_u
    out = {"one": 1, "sub_pass": max(1, rpb - 1), "trip_minus_1": u * rpb - 1,
           "trip_plus_1": u * rpb + 1}
    for r in range(1, u):
        out[f"second_trip_{r}"] = (u + r) * rpb
    for M in out.values():
        assert reduce_blocks(M, C, k) == (1, "rows"), (C, M)
    # (rpb = 1: a single thread per channel group owns every row)
    assert last_trip_rows(out["trip_minus_1"], C, k) == ({u - 1, u} if rpb > 1 else {u - 1})
    assert last_trip_rows(out["trip_plus_1"], C, k) == ({1, u} if rpb > 1 else {1})
    for r in range(1, u):
        assert last_trip_rows(out[f"second_trip_{r}"], C, k) == {r}
    return out


def rows_sum16_loops(P):
    """(trips of the 8-deep loop, trips of the tail loop) of rows_sum16's row group 0."""
    p, deep, tail = 0, 0, 0
    while p + 7 * 16 < P:
        p += 8 * 16
        deep += 1
    while p < P:
        p += 16
        tail += 1
    return deep, tail


def cap_cases(k):
    """(name, C, M, small_ranges) of the reduction's grid-limit cases, each asserted through the
    mirrored launcher formula (the GPU test asserts the same through the exported function)."""
    cases = []
    # the atomic budget binds: C = 2048, just above budget * row_iters rows
    C = 2048
    G = k.atomic_budget // (3 * C)
    M = G * k.row_iters + 17
    assert reduce_blocks(M, C, k) == (G, "budget") and G > k.min_blocks
    cases.append(("budget", C, M, False))
    # C = 4096: two channel passes, and the budget is still above the floor
    C = 4096
    G = k.atomic_budget // (3 * C)
    M = G * k.row_iters + 5
    assert reduce_blocks(M, C, k) == (G, "budget") and row_map(C, k)[2] == 2
    cases.append(("budget_2pass", C, M, False))
    # the floor binds only once budget / (3 C) < min_blocks: the smallest such C % 8 == 0
    C = (k.atomic_budget // (3 * k.min_blocks)) // 8 * 8 + 8
    M = k.min_blocks * k.row_iters + 9
    assert k.atomic_budget // (3 * C) < k.min_blocks
    assert reduce_blocks(M, C, k) == (k.min_blocks, "floor")
    cases.append(("floor", C, M, False))
    # the block cap: C = 64, just above reduce_blocks * row_iters * rpb rows (about 2^19)
    C = 64
    M = k.reduce_blocks * k.row_iters * row_map(C, k)[1] + 77
    assert reduce_blocks(M, C, k) == (k.reduce_blocks, "cap")
    cases.append(("block_cap", C, M, True))
    return cases


def det_cases(k):
    """(name, C, M) whose deterministic collect takes each path of bn_bwd_collect_rows."""
    cases = []
    # G <= 4 * det_chunk_rows: rows_sum16 with both its loops running and a tail in each
    C = 2048
    G = 128 + 5
    M = (G - 1) * k.row_iters + 3
    assert reduce_blocks(M, C, k) == (G, "rows") and G <= 4 * k.det_chunk_rows
    deep, tail = rows_sum16_loops(G)
    assert deep >= 1 and tail >= 1 and G % 16 != 0
    cases.append(("sum16_tails", C, M))
    # G > 4 * det_chunk_rows and no multiple of it: det_chunk_sums with a short last chunk
    C = 64
    rpb = row_map(C, k)[1]
    M = (4 * k.det_chunk_rows + 1) * k.row_iters * rpb + 100
    G, why = reduce_blocks(M, C, k)
    assert why == "rows" and G > 4 * k.det_chunk_rows and G % k.det_chunk_rows != 0
    cases.append(("chunk_sums", C, M))
    return cases


def reduce_chain(M, C, k, det):
    """Longest chain of fp32 additions in bn_act_bwd_reduce: a thread's rows, the rpb row groups
    of the LDS transpose, then either the blocks that add into one replica row and the replica
    sum, or the fixed-order collect (chunk sums of det_chunk_rows rows in 4 groups, then
    rows_sum16's groups and their 16 sums)."""
    _, rpb, _ = row_map(C, k)
    G, _ = reduce_blocks(M, C, k)
    chain = cdiv(M, G * rpb) + rpb
    if not det:
        return chain + cdiv(G, k.replicas) + k.replicas
    P = G
    if P > 4 * k.det_chunk_rows:
        chain += k.det_chunk_rows // 4 + 4
        P = cdiv(P, k.det_chunk_rows)
    return chain + cdiv(P, 16) + 16


# ------------------------------------------------------------------------------ constructions
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _cycle(values, C, mul, add):
    """values[(mul*c + add) % n] per channel: every value (and, with different strides, every
    pairing within a few channels) is present from C = 8 on, without leaving it to a seed."""
    v = torch.tensor(values, dtype=torch.float64)
    return v[(torch.arange(C) * mul + add) % len(values)]


K_VALUES = [0.0, 0.25, -0.25, 0.5, -0.5]
COUNT = 4096


@functools.lru_cache(maxsize=2)
def exact_inputs(C, M, small=False):
    """float64 CPU tensors of one exact case (forward, reduce and apply share them).  small: the
    shrunken ranges for M beyond 2^17."""
    g = _gen("exact", C, M)
    a = 1 if small else 4
    d = SimpleNamespace(C=C, M=M, small=small)
    d.y, d.r, d.y2 = (_ints(g, -2 if small else -4, 2 if small else 4, M, C) for _ in range(3))
    d.dz = _ints(g, -a, a, M, C)
    d.z = _ints(g, 0, 1, M, C) * 2.0                       # a ReLU output: 0 | 2
    d.zneg = d.z - 2.0 * _ints(g, 0, 1, M, C)              # relu = False must ignore z: -2 | 0 | 2
    for row in (M - 1, M // 2):        # the rows the reduction's mutants drop / repeat count
        d.dz[row, 0], d.z[row, 0], d.zneg[row, 0] = 1.0, 2.0, 2.0
        d.y[row, 0] = d.y2[row, 0] = 2.0
    # forward coefficients
    d.scale = _cycle([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], C, 1, 0)
    d.bias = _cycle([-3.0, -1.0, 0.0, 1.0, 2.0], C, 1, 1)
    d.rscale = _cycle([-1.0, 0.5, 1.0], C, 1, 0)
    d.rbias = _cycle([-2.0, 0.0, 1.0], C, 2, 0)
    # backward statistics
    mu = [-1.0, 0.0, 1.0] if small else [-2.0, -1.0, 0.0, 1.0, 2.0]
    inv = [1.0, 2.0] if small else [0.5, 1.0, 2.0]
    d.mean, d.mean2 = _cycle(mu, C, 1, 1), _cycle(mu, C, 1, 3)
    d.invstd, d.invstd2 = _cycle(inv, C, 1, 0), _cycle(inv, C, 2, 1)
    d.gamma = _cycle([0.5, -0.5, 1.0, -1.0, 2.0], C, 1, 2)
    d.gamma2 = _cycle([0.5, -0.5, 1.0, -1.0, 2.0], C, 3, 0)
    d.k1, d.k2, d.k22 = _cycle(K_VALUES, C, 1, 1), _cycle(K_VALUES, C, 2, 1), _cycle(K_VALUES, C, 3, 2)
    d.count = COUNT
    d.sum_g, d.sum_gx, d.sum_gx2 = d.k1 * COUNT, d.k2 * COUNT, d.k22 * COUNT
    # |g| * |y - mean| * invstd and the dyadic step of the reduction's terms
    d.term_max = a * ((2 if small else 4) + max(mu)) * max(inv)
    d.term_step = min(inv)
    return d


def reduce_exact_bound(d):
    """Per channel, sum of |terms| in units of the smallest dyadic step (a priori, from the ranges)."""
    return d.M * d.term_max / d.term_step


def assert_exact(ref, units, stored=None):
    """ref is representable in fp32 (and in ``stored``); ``units`` = sum of the terms' magnitudes
    over the smallest dyadic step of any term or partial sum, which must stay below 2^24."""
    assert torch.equal(ref, ref.float().double())
    if stored is not None:
        assert torch.equal(ref, ref.to(stored).double())
    units = units.max().item() if torch.is_tensor(units) else units
    assert units < EXACT, units


# ------------------------------------------------------------------------------ float64 references
def ref_fwd(y, scale, bias, r, rscale, rbias, relu, mutant=None):
    """(z, T): z = act(y*scale + bias [+ r | + r*rscale + rbias]) in float64 and the sum of the
    terms' magnitudes.  mutant: 'bias' (dropped), 'res' (residual dropped), 'res_affine' (the
    residual's scale and bias ignored)."""
    y = y.double()
    sc, bi = scale.double(), bias.double()
    if mutant == "bias":
        bi = torch.zeros_like(bi)
    z = y * sc + bi
    T = (y * sc).abs() + bi.abs()
    if r is not None and mutant != "res":
        rr = r.double()
        if rscale is not None and mutant != "res_affine":
            z = z + rr * rscale.double() + rbias.double()
            T = T + (rr * rscale.double()).abs() + rbias.double().abs()
        else:
            z = z + rr
            T = T + rr.abs()
    if relu:
        z = torch.relu(z)
    return z, T


def masked_g(dz, z, relu):
    g = dz.double()
    return g * (z.double() > 0) if relu else g


def ref_reduce(dz, z, y, mean, invstd, relu, y2=None, mean2=None, invstd2=None, mutant=None):
    """Namespace sg, sgx, sgx2 (float64 per channel) and ag, agx, agx2, the sums of magnitudes.
    mutant: 'drop_row' (the last row missing), 'dup_row' (row M//2 counted twice)."""
    g = masked_g(dz, z, relu)
    w = torch.ones(g.shape[0], 1, dtype=torch.float64, device=g.device)
    if mutant == "drop_row":
        w[-1] = 0.0
    elif mutant == "dup_row":
        w[g.shape[0] // 2] = 2.0
    o = SimpleNamespace(sgx2=None, agx2=None)
    t = g * w
    o.sg, o.ag = t.sum(0), t.abs().sum(0)
    t = g * (y.double() - mean.double()) * invstd.double() * w
    o.sgx, o.agx = t.sum(0), t.abs().sum(0)
    if y2 is not None:
        t = g * (y2.double() - mean2.double()) * invstd2.double() * w
        o.sgx2, o.agx2 = t.sum(0), t.abs().sum(0)
    return o


def _branch(g, y, mean, invstd, gamma, k1, k2):
    """dy = A*g + B*y + Cc as bn_bwd_apply_kernel writes it, and T = sum of its terms' magnitudes."""
    a = gamma * invstd
    B = -a * invstd * k2
    c1, c2 = -a * k1, a * invstd * k2 * mean
    return a * g + B * y + (c1 + c2), (a * g).abs() + (B * y).abs() + c1.abs() + c2.abs()


def ref_apply(dz, z, y, mean, invstd, gamma, sum_g, sum_gx, count, relu, y2=None, mean2=None,
              invstd2=None, gamma2=None, sum_gx2=None, mutant=None):
    """Namespace dy, T, g (the masked gradient = dres), dy2, T2; all float64.
    dy = gamma*invstd*(g - k1 - xhat*k2), k1 = sum_g/count, k2 = sum_gx/count.
    mutant: 'k1' | 'k2' | 'mean' | 'mean2' | 'k22' — that quantity taken as zero."""
    f = lambda t: None if t is None else t.double()
    zero = lambda t, name: torch.zeros_like(t) if mutant == name else t
    g = masked_g(dz, z, relu)
    k1 = zero(f(sum_g) / count, "k1")
    k2 = zero(f(sum_gx) / count, "k2")
    o = SimpleNamespace(g=g, dy2=None, T2=None)
    o.dy, o.T = _branch(g, f(y), zero(f(mean), "mean"), f(invstd), f(gamma), k1, k2)
    if y2 is not None:
        k22 = zero(f(sum_gx2) / count, "k22")
        o.dy2, o.T2 = _branch(g, f(y2), zero(f(mean2), "mean2"), f(invstd2), f(gamma2), k1, k22)
    return o


def ref_finalize(psum, psq, count, shift, gamma, beta, eps):
    """Namespace of float64 mean, var (clamped), invstd, scale, bias and the bound on invstd."""
    a, b = psum.double().sum(0), psq.double().sum(0)
    P = psum.shape[0]
    ms = a / count
    ex2 = b / count
    o = SimpleNamespace()
    o.raw_var = ex2 - ms * ms
    o.var = o.raw_var.clamp_min(0.0)
    o.mean = ms + shift.double()
    o.invstd = torch.rsqrt(o.var + eps)
    o.scale = gamma.double() * o.invstd
    o.bias = beta.double() - o.mean * o.scale
    # fp32 error of var = fl(fl(b)*fl(1/n)) - fl(ms*ms): b and a are P-term sums (P roundings,
    # relative to the sum of magnitudes), 1/n and the product round once each; ms enters squared,
    # so its P + 2 roundings count twice, plus the square and the subtraction.
    sb = psq.double().abs().sum(0) / count
    sa = psum.double().abs().sum(0) / count
    dvar = U24 * ((P + 3) * sb + (2 * (P + 2) + 2) * sa * sa)
    # invstd = (var + eps)^-1/2: half the relative error of var + eps, the rounding of eps and of
    # the sum, and 2 ulp for the hardware reciprocal square root
    # Where the true difference is negative by more than that error, fp32 clamps too: var = 0.
    dvar = torch.where(o.raw_var < -dvar, torch.zeros_like(dvar), dvar)
    o.invstd_tol = o.invstd * (0.5 * dvar / (o.var + eps) + 8 * U24)
    return o


# ------------------------------------------------------------------------------ bounds
def elementwise_bound(ref, T, dtype):
    b = 16 * U24 * T
    return b + 2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else b


def reduce_bound(abs_terms, chain):
    return (chain + 3) * U24 * abs_terms


def worst(out, ref, bound):
    """Largest |out - ref| / bound (0/0 counts as 0): <= 1 passes."""
    d = (out.double() - ref).abs()
    q = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return q.max().item()


# ------------------------------------------------------------------------------ random cases
RANDOM_CASES = [("C40", 40, 301, 0.0), ("C64", 64, 1500, 0.0), ("C1000", 1000, 37, 0.0),
                ("C2056", 2056, 19, 0.0), ("offset1000", 64, 700, 1000.0)]


@functools.lru_cache(maxsize=2)
def random_inputs(name, C, M, offset, dtype):
    """One random case with realistic statistics: mean / invstd are those of y itself (of the
    values as stored in ``dtype``), sums are the float64 reductions rounded to fp32, and every
    per-channel vector is the fp32 one that kernel and reference both get."""
    g = _gen("random", name, C, M)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = SimpleNamespace(C=C, M=M, dtype=dtype, count=M)
    spread = torch.rand(C, generator=g) * 2 + 0.5
    d.y = (rn(M, C) * spread + rn(C) * (0.0 if offset else 1.0) + offset).to(dtype)
    d.y2 = (rn(M, C) * spread.flip(0) + rn(C)).to(dtype)
    d.r = rn(M, C).to(dtype)
    d.dz = rn(M, C).to(dtype)
    st = lambda t: (t.double().mean(0).float(),
                    torch.rsqrt(t.double().var(0, unbiased=False) + EPS).float())
    (d.mean, d.invstd), (d.mean2, d.invstd2) = st(d.y), st(d.y2)
    d.gamma, d.gamma2 = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    d.beta, d.beta2 = rn(C) * 0.5, rn(C) * 0.5
    d.scale, d.rscale = d.gamma * d.invstd, d.gamma2 * d.invstd2
    d.bias, d.rbias = d.beta - d.mean * d.scale, d.beta2 - d.mean2 * d.rscale
    # z: what the two-branch forward stores (any tensor would do: both sides read the same one)
    d.z = ref_fwd(d.y, d.scale, d.bias, d.y2, d.rscale, d.rbias, True)[0].to(dtype)
    red = ref_reduce(d.dz, d.z, d.y, d.mean, d.invstd, True, d.y2, d.mean2, d.invstd2)
    d.sum_g, d.sum_gx, d.sum_gx2 = red.sg.float(), red.sgx.float(), red.sgx2.float()
    return d


# ------------------------------------------------------------------------------ fp32 models
def model_fwd_fp32(y, scale, bias, r, rscale, rbias, relu, out_dtype):
    """bn_act_fwd_kernel's arithmetic in fp32 (no contraction), stored as out_dtype."""
    v = y.float() * scale + bias
    if r is not None:
        v = v + (r.float() * rscale + rbias if rscale is not None else r.float())
    return (torch.relu(v) if relu else v).to(out_dtype)


def model_apply_fp32(g, y, mean, invstd, gamma, sum_g, sum_gx, count, out_dtype):
    """One branch of bn_bwd_apply_kernel in fp32, operation by operation."""
    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(count), dtype=torch.float32)
    a = gamma * invstd
    k1, k2 = sum_g * inv_n, sum_gx * inv_n
    B = -a * invstd * k2
    Cc = -a * k1 + a * invstd * k2 * mean
    return (a * g.float() + B * y.float() + Cc).to(out_dtype)


def model_reduce_fp32(terms, C, k, det):
    """Sum fp32 ``terms`` [M, C] over rows in the kernel's own order of additions: a thread's rows
    in sequence, the row groups of a block in sequence, then blocks into replica rows and the
    replica rows (atomic mode, blocks taken in index order) or, deterministic, the chunk sums and
    rows_sum16's 16 groups."""
    M = terms.shape[0]
    _, rpb, _ = row_map(C, k)
    G, _ = reduce_blocks(M, C, k)
    J = cdiv(M, G * rpb)
    x = torch.zeros(J * G * rpb, C, dtype=torch.float32)
    x[:M] = terms.float()
    x = x.reshape(J, G, rpb, C)
    acc = torch.zeros(G, rpb, C)
    for j in range(J):
        acc = acc + x[j]
    blk = torch.zeros(G, C)
    for q in range(rpb):
        blk = blk + acc[:, q]

    def seq(rows):                      # rows [n, C] added in index order
        s = torch.zeros(C)
        for row in rows:
            s = s + row
        return s

    if not det:
        return seq(torch.stack([seq(blk[r::k.replicas]) for r in range(k.replicas)]))
    if G > 4 * k.det_chunk_rows:
        chunks = []
        for c0 in range(0, G, k.det_chunk_rows):
            ch = blk[c0:c0 + k.det_chunk_rows]
            p = [seq(ch[q::4]) for q in range(4)]
            chunks.append(((p[0] + p[1]) + p[2]) + p[3])
        blk = torch.stack(chunks)
    return seq(torch.stack([seq(blk[q::16]) if q < blk.shape[0] else torch.zeros(C)
                            for q in range(16)]))


# ------------------------------------------------------------------------------ bn_finalize
NEG_VAR_CHANNEL = 3


def finalize_inputs(C, count, P):
    """Replica slabs [P, C] of shifted sums with per-channel mean ~ N(0,1) and variance in
    [0.5, 1.5].  Channel NEG_VAR_CHANNEL holds exact values with E[x^2] - ms^2 = -2^-10 (ms = 3,
    E[x^2] = 9 - 2^-10, every sum exact in fp32): the clamp must give var = 0."""
    g = _gen("finalize", C, count)
    m, v = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    psum = (m + 0.1 * torch.randn(P, C, generator=g)) * (count / P)
    psq = (m * m + v * (1 + 0.1 * torch.randn(P, C, generator=g))) * (count / P)
    psum[:, NEG_VAR_CHANNEL] = 3.0 * count / P
    psq[:, NEG_VAR_CHANNEL] = (9.0 - 2.0 ** -10) * count / P
    d = SimpleNamespace(psum=psum, psq=psq, count=count)
    d.shift = torch.randn(C, generator=g) * 0.1
    d.gamma, d.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    return d


def model_finalize_fp32(d, eps):
    """bn_finalize_kernel in fp32: (mean, var, invstd)."""
    a, b = torch.zeros_like(d.psum[0]), torch.zeros_like(d.psq[0])
    for p in range(d.psum.shape[0]):
        a, b = a + d.psum[p], b + d.psq[p]
    inv = torch.tensor(1.0) / torch.tensor(float(d.count))
    ms = a * inv
    var = (b * inv - ms * ms).clamp_min(0.0)
    return ms + d.shift, var, torch.rsqrt(var + torch.tensor(eps))
