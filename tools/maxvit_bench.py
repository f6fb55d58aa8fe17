"""The MaxViT kernels alone at the four stage shapes of maxvit_t, B = 64, bf16, against the ATen
composition that ``MaxVit.reference_forward`` uses, on the same tensors.

    partition_attention fwd / fwd+bwd, block and grid   hip (relattn.hip)  vs  aten: partition
        (and swap), two einsums, bias gather, softmax, departition (autograd backward)
    bn_act_pool gelu fwd (with the pool)                hip (se.hip)       vs  aten: affine,
        F.gelu, mean over (h, w)

Maps 56^2 x 2 heads, 28^2 x 4, 14^2 x 8, 7^2 x 16, score scale C^-1/2; the GELU pass at the
MBConv widths 4C of the same maps.  All candidates of a shape run in ONE process on the same
buffers, alternated ``--reps`` times (at least four); a timed loop is ``--iters`` calls between two
device events after ``--warmup`` untimed calls (tools/swin_bench.py's scheme).  ``--resources``
instead compiles relattn.hip and prints the compiler's VGPR / AGPR / LDS / scratch figures per
kernel (no GPU needed; profiles/maxvit_resources.txt).
``grid_over_block`` is grid mode's time over block mode's at the same shape: the cost of the
strided gather.

Usage: python tools/maxvit_bench.py [--batch 64] [--reps 4] [--iters 10]
                                    [--out profiles/maxvit_kernels.txt] | --resources
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

STAGES = [(56, 2), (28, 4), (14, 8), (7, 16)]


def main(argv=None) -> int:
    from tools.swin_bench import resources
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=10, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls per candidate")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 4)
    if a.resources:
        for rec in resources("relattn.hip"):
            print(json.dumps(rec))
        return 0

    import torch
    import torch.nn.functional as F
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import _ref
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("maxvit_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"maxvit_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2
    bf, B, lines = torch.bfloat16, a.batch, []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def aten_attention(qkv, table, rel, hw, H, mode, scale):
        """reference_forward's attention on the packed projection, bf16."""
        p = 7 if mode == "block" else hw // 7
        n = hw // p
        x = qkv.view(B, n, p, n, p, 3, H, 32).permute(5, 0, 1, 3, 2, 4, 6, 7)
        x = x.reshape(3, B, n * n, p * p, H, 32)
        if mode == "grid":
            x = x.swapaxes(-3, -4)
        q, k, v = x[0], x[1] * scale, x[2]
        dot = torch.einsum("bgihd,bgjhd->bghij", q, k) + table[rel].permute(2, 0, 1).to(bf)
        o = torch.einsum("bghij,bgjhd->bgihd", F.softmax(dot, -1), v)
        if mode == "grid":
            o = o.swapaxes(-3, -4)
        o = o.reshape(B, n, n, p, p, H * 32).permute(0, 1, 3, 2, 4, 5)
        return o.reshape(B * hw * hw, H * 32)

    def timed(cands):
        for fn in cands.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in cands}
        for _ in range(a.reps):
            for k, fn in cands.items():
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        return us

    def report(shape, us, extra=None):
        keys = list(us)
        for i in range(0, len(keys), 2):
            k, ref = keys[i], keys[i + 1]
            for name in (k, ref):
                med = statistics.median(us[name])
                rec = {"shape": shape, "candidate": name, "us_per_call": round(med, 2),
                       "us_all": [round(v, 2) for v in us[name]]}
                if name == k:
                    rec["vs"] = ref
                    rec["speedup"] = round(statistics.median(us[ref]) / med, 3)
                    rec["faster_in_every_alternation"] = all(
                        h < r for h, r in zip(us[k], us[ref]))
                emit(rec)
        if extra:
            emit(extra(us))

    with ClockSampler(0) as cs:
        for hw, H in STAGES:
            torch.manual_seed(0)
            T, C = B * hw * hw, H * 32
            scale = C ** -0.5
            qkv = torch.randn(T, 3 * C, device="cuda").to(bf)
            do = torch.randn(T, C, device="cuda").to(bf)
            rel = _ref.window_geometry(7, 7, 0, "cuda")[1]
            table = torch.randn(169, H, device="cuda") * 0.1
            dt = torch.zeros(169 * H, device="cuda")
            qa, ta = qkv.clone().requires_grad_(), table.clone().requires_grad_()
            cands = {}
            for mode in ("block", "grid"):
                def hip_f(mode=mode):
                    return K.partition_attention_fwd(qkv, table, B, hw, hw, H, mode, scale)

                def hip_fb(mode=mode):
                    hip_f(mode)
                    K.partition_attention_bwd(do, qkv, table, B, hw, hw, H, mode, scale, dt)

                def aten_f(mode=mode):
                    return aten_attention(qkv, table, rel, hw, H, mode, scale)

                def aten_fb(mode=mode):
                    qa.grad = ta.grad = None
                    aten_attention(qa, ta, rel, hw, H, mode, scale).backward(do)

                cands.update({f"relattn_{mode}_fwd/hip": hip_f, f"relattn_{mode}_fwd/aten": aten_f,
                              f"relattn_{mode}_fwd_bwd/hip": hip_fb,
                              f"relattn_{mode}_fwd_bwd/aten": aten_fb})

            def ratio(us, hw=hw, H=H):
                med = {k: statistics.median(v) for k, v in us.items()}
                return {"shape": [B, hw, hw, H], "grid_over_block": {
                    p: round(med[f"relattn_grid_{p}/hip"] / med[f"relattn_block_{p}/hip"], 3)
                    for p in ("fwd", "fwd_bwd")}}

            report([B, hw, hw, H], timed(cands), ratio)
            # BatchNorm + GELU + pool at the MBConv width of this map
            y = torch.randn(B, hw, hw, 4 * C, device="cuda").to(bf)
            sc, bi = torch.rand(4 * C, device="cuda") + 0.5, torch.randn(4 * C, device="cuda")

            def aten_gelu():
                z = F.gelu(y * sc.to(bf) + bi.to(bf))
                return z, z.float().mean((1, 2))

            report([B, hw, hw, 4 * C], timed({
                "bn_gelu_pool_fwd/hip": lambda: K.bn_act_pool_fwd(y, sc, bi, "gelu", True),
                "bn_gelu_pool_fwd/aten": aten_gelu}))
    emit({"batch": B, "dtype": "bf16", "gpu_clocks": cs.summary(), "reps": a.reps,
          "iters": a.iters})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
