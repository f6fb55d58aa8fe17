"""Shared by test_large_batch_optim_cpu.py / _gpu.py: the small synthetic flat space, the
per-tensor float64 reference run (mipipe.ops._ref rules on separate tensors) and the optimizer
run it is compared with."""
import torch

from mipipe.ops import _ref

CH = 8192
NSEG = 40
I_BIG, I_MID, I_PAD, I_ZERO_G, I_ZERO_W = 0, 1, 2, 3, 4
PAD_ROWS = 32


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def shapes():
    """40 tensors: one of 65·CH elements, one of CH + 64, one registered with padded rows
    (30 -> 32 rows of 48), 64-element matrices (one gets zero gradients, one is all zero) and
    1-D tensors of 64, 37 and 100 elements (the last two end in alignment padding)."""
    s = [(520, 1024), (129, 64), (30, 48), (8, 8), (4, 16)]
    s += [(64,), (37,), (100,), (64,), (1,)]
    s += [(8, 8)] * (NSEG - len(s))
    return s


def make_params(device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i, sh in enumerate(shapes()):
        w = torch.randn(*sh, generator=g) * (0.05 + 0.01 * (i % 7))
        if i == I_ZERO_W:
            w.zero_()
        p = torch.nn.Parameter(w.to(device))
        if i == I_PAD:
            p._mipipe_pad_rows = PAD_ROWS
        ps.append(p)
    return ps


def make_grads(steps, seed=1, scale=1.0):
    """[step][tensor] CPU fp32 gradients; tensor I_ZERO_G's are all zero."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        gs = [torch.randn(*sh, generator=g) * scale * (0.01 + 0.003 * (i % 5))
              for i, sh in enumerate(shapes())]
        gs[I_ZERO_G].zero_()
        out.append(gs)
    return out


def lars_hp(**kw):
    hp = dict(kind="lars", sched=("poly", 0.5, 2, 6, 0.01), momentum=0.9, weight_decay=1e-3,
              tc=0.02, eps=1e-8, max_norm=None, exclude_1d=True, grad_scale=1.0)
    hp.update(kw)
    return hp


def lamb_hp(**kw):
    hp = dict(kind="lamb", sched=("cosine", 0.01, 1, 8, 1e-4), betas=(0.9, 0.999), eps=1e-6,
              weight_decay=0.01, max_norm=None, exclude_1d=True, grad_scale=1.0)
    hp.update(kw)
    return hp


def run_ref(ws, grads, hp, dtype=torch.float64):
    """The _ref rules per tensor on separate tensors of ``dtype``.  -> dict of flat results."""
    kind, base, W, T, end = hp["sched"]
    w = [x.detach().cpu().to(dtype).clone() for x in ws]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    ratios, norms = [], []
    for k, gs in enumerate(grads):
        gs = [x.to(dtype) for x in gs]
        lr = _ref.lr_schedule(kind, base, W, T, end, k)
        norm, clip = _ref.clip_coef(gs, hp["grad_scale"], hp["max_norm"])
        gsc = hp["grad_scale"] * clip
        rs = []
        for i in range(len(w)):
            skip = hp["exclude_1d"] and w[i].dim() <= 1
            wd = 0.0 if skip else hp["weight_decay"]
            if hp["kind"] == "lars":
                r = _ref.lars_step(w[i], gs[i], m[i], lr, hp["momentum"], wd, hp["tc"],
                                   hp["eps"], not skip, gsc)
            else:
                r = _ref.lamb_step(w[i], gs[i], m[i], v[i], lr, hp["betas"][0], hp["betas"][1],
                                   hp["eps"], wd, k + 1, not skip, gsc)
            rs.append(float(r))
        ratios.append(torch.tensor(rs, dtype=torch.float64))
        norms.append(float(norm))
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])  # noqa: E731
    return dict(p=cat(w), m=cat(m), v=cat(v), ratios=ratios, norms=norms)


def make_opt(params, hp):
    from mipipe.optim import LAMB, LARS, LRSchedule
    sched = LRSchedule(*hp["sched"])
    if hp["kind"] == "lars":
        return LARS(params, sched, momentum=hp["momentum"], weight_decay=hp["weight_decay"],
                    trust_coefficient=hp["tc"], eps=hp["eps"], max_grad_norm=hp["max_norm"],
                    exclude_1d=hp["exclude_1d"])
    return LAMB(params, sched, betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                max_grad_norm=hp["max_norm"], exclude_1d=hp["exclude_1d"])


def set_grads(opt, params, gs):
    for p, g in zip(params, gs):
        opt.space.grad_view(p).copy_(g)


def run_opt(params, grads, hp, opt=None):
    """The optimizer over the flat space.  -> (dict like run_ref's, optimizer); ratios are
    reordered from flat order to the order of ``params``."""
    opt = opt or make_opt(params, hp)
    pos = {id(p): s for s, p in enumerate(opt.space.order)}
    perm = torch.tensor([pos[id(p)] for p in params])
    ratios, norms = [], []
    for gs in grads:
        set_grads(opt, params, gs)
        opt.step(grad_scale=hp["grad_scale"])
        ratios.append(opt.last_trust_ratios().detach().cpu().double()[perm])
        n = opt.last_grad_norm()
        norms.append(None if n is None else float(n))
    cat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])  # noqa: E731
    names = ["momentum_buffer"] if hp["kind"] == "lars" else ["exp_avg", "exp_avg_sq"]
    st = [cat([opt.state[p][n] for p in params]) for n in names]
    out = dict(p=cat(params), m=st[0], v=st[-1], ratios=ratios, norms=norms)
    return out, opt


def padding_mask(space):
    """True where the flat buffer is padding: alignment tails and reserved pad rows."""
    mask = torch.ones(space.numel, dtype=torch.bool)
    for a, _, p in space.ranges():
        mask[a:a + p.numel()] = False  # contiguous parameters: the first numel() are real
    return mask
