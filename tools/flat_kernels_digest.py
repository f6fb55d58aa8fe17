"""Bit digests of the flat-buffer kernels (csrc/kernels/optim.hip, ema.hip): SGD, AdamW, LARS,
LAMB, the weight EMA update / swap and the two EMA buffer-table operations.

The contracts of these kernels against ``mipipe.ops._ref`` are tolerances, so a refactor that
must keep every bit is checked against the build it refactors instead: run this file on both
builds and compare the outputs line by line.  Inputs come from CPU generators with fixed seeds;
only ``native()`` entry points are called (LARS and LAMB through ``mipipe.optim``, whose Python
builds their device tables), so one file serves any two builds whose entry points agree.  Every
case runs with the streaming bit (1024) of ``set_nt_store`` set and cleared and prints

    <case> <sha256 over every output buffer>

Usage: python tools/flat_kernels_digest.py [--out FILE]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZES = (4, 1028, 12288)  # one item; 257 items (one live second slot of AdamW's unroll 2); 3 blocks


def digest(*tensors) -> str:
    import torch
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().contiguous().cpu()
        h.update(str((t.dtype, tuple(t.shape))).encode())
        h.update(t.view(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)

    import torch
    from mipipe.ops._native import load_error, native, native_available

    if not torch.cuda.is_available():
        print("flat_kernels_digest: no GPU", file=sys.stderr)
        return 2
    if not native_available():
        print(f"flat_kernels_digest: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2
    C = native()
    dev = torch.device("cuda", 0)
    lines = []

    def emit(case, *tensors):
        torch.cuda.synchronize()
        s = f"{case} {digest(*tensors)}"
        print(s, flush=True)
        lines.append(s)

    def rand(n, seed, scale=1.0):
        return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)

    def sgd(tag):
        for n in SIZES:
            for name, mom, nesterov in (("mom", 0.9, False), ("plain", 0.0, False),
                                        ("nesterov", 0.9, True)):
                for shadow in (True, False):
                    p, g = rand(n, 1), rand(n, 2, 0.1)
                    m = torch.zeros(n, device=dev) if mom != 0 else g  # as mipipe.optim.SGD passes it
                    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev) if shadow else None
                    for k in range(3):  # a first step and two later ones
                        if mom != 0:
                            g.copy_(rand(n, 10 + k, 0.1))
                        C.sgd_step(p, g, m, sh, 0.1, mom, 0.0, 1e-4, nesterov, k == 0, 0.5)
                        emit(f"sgd/{tag}/n{n}/{name}/shadow{int(shadow)}/step{k}", p, m, sh)

    def adamw(tag):
        for n in SIZES:
            for devstep in (False, True):
                p, g = rand(n, 3), rand(n, 4, 0.1)
                m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
                sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
                t = torch.zeros(1, dtype=torch.int32, device=dev) if devstep else None
                for k in (1, 2, 3):
                    g.copy_(rand(n, 20 + k, 0.1))
                    if t is not None:
                        t.fill_(k)
                    C.adamw_step(p, g, m, v, sh, 1e-3, 0.9, 0.999, 1e-8, 0.01, k, 0.5, step_dev=t)
                    emit(f"adamw/{tag}/n{n}/devstep{int(devstep)}/step{k}", p, m, v, sh)

    def large_batch(tag):
        import large_batch_common as lb
        cfgs = [("lars", lb.lars_hp()), ("lars_clip", lb.lars_hp(max_norm=0.05)),
                ("lars_notc", lb.lars_hp(tc=None)), ("lamb", lb.lamb_hp()),
                ("lamb_clip", lb.lamb_hp(max_norm=0.05))]
        grads = lb.make_grads(4)
        for name, hp in cfgs:
            params = lb.make_params(dev)
            opt = lb.make_opt(params, hp)
            assert opt.space.shadow is not None
            for k, gs in enumerate(grads):
                lb.set_grads(opt, params, gs)
                opt.step(grad_scale=0.5)
                st = [opt._flat_state(s) for s in opt._state_names]
                emit(f"{name}/{tag}/step{k}", opt.space.flat, *st, opt.space.shadow, opt._scal,
                     opt._ratio, opt._part, opt._segtot)

    def ema_flat(tag, name, p, shadow):
        n = p.numel()
        for every in (1, 3):
            for warmup in (True, False):
                e = rand(n, 5)
                t = torch.zeros(1, dtype=torch.int32, device=dev)
                scal = torch.zeros(1, device=dev)
                for call in range(1, 7):
                    t.fill_(call)
                    C.ema_update(p, e, t, every, 1.0 - 0.99, warmup, scal)
                    emit(f"ema_update/{tag}/{name}/every{every}/warmup{int(warmup)}/call{call}",
                         e, scal, p)
        for sh in ((shadow, None) if shadow is not None else (None,)):
            q, e = p.clone(), rand(n, 6)
            s = sh.clone() if sh is not None else None
            for k in range(2):
                C.ema_swap(q, e, s)
                emit(f"ema_swap/{tag}/{name}/shadow{int(sh is not None)}/swap{k}", q, e, s)

    def ema(tag):
        from mipipe.optim import SGD
        from test_model_ema_gpu import Bag
        model = Bag().to(dev)
        model.emb._mipipe_pad_rows = 8
        space = SGD(model.parameters(), lr=0.1, shadow_dtype="auto").space
        ema_flat(tag, "bag", space.flat, space.shadow)
        ema_flat(tag, "n64", rand(64, 7), torch.zeros(64, dtype=torch.bfloat16, device=dev))
        # buffer table: rows {address, offset into the EMA's copy, length}
        bufs = [rand(k, 30 + k) for k in (1, 7, 64, 300, 1024)]
        offs, rows = 0, []
        for b in bufs:
            rows.append([b.data_ptr(), offs, b.numel()])
            offs += b.numel()
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        eb = rand(offs, 8)
        t = torch.zeros(1, dtype=torch.int32, device=dev)
        for call in range(1, 5):
            t.fill_(call)
            C.ema_buffers_update(table, eb, t, 2, 1.0 - 0.9, True)
            emit(f"ema_buffers_update/{tag}/call{call}", eb, *bufs)
        for k in range(2):
            C.ema_buffers_swap(table, eb)
            emit(f"ema_buffers_swap/{tag}/swap{k}", eb, *bufs)

    saved = C.get_nt_store()
    try:
        for tag, mask in (("stream", saved | 1024), ("cached", saved & ~1024)):
            C.set_nt_store(mask)
            sgd(tag)
            adamw(tag)
            large_batch(tag)
            ema(tag)
    finally:
        C.set_nt_store(saved)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
