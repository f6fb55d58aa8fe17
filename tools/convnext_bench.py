"""The ConvNeXt kernels alone at the stage shapes of convnext_tiny and convnext_large, B = 64,
bf16, against the paths they replace.

    dwconv7 fwd / dgrad / wgrad   hip (dwconv7.hip)   vs  the generic depthwise kernels of
                                                          vision.hip (gconv_* with groups = C)
    scale_residual fwd            hip                 vs  aten: res + (f * gamma) * s
    scale_residual bwd            hip                 vs  aten: df, the dgamma and bias column sums

Maps 56^2 / 28^2 / 14^2 / 7^2 at widths 96 / 192 / 384 / 768 (tiny) and 192 / 384 / 768 / 1536
(large).  All candidates run in ONE process on the same buffers, alternated ``--reps`` times (at
least four); a timed loop is ``--iters`` calls between two device events after ``--warmup``
untimed calls, and the shader clock is sampled meanwhile (mipipe/obs/clocks.py).  Per candidate:
the µs per call of every alternation, the median, the bytes the operation has to move (every
tensor it must read or write once) and the TB/s that gives.  The smaller working sets fit the
memory-side cache, so back-to-back calls read partly from it: an upper bound for a training step.

Usage: python tools/convnext_bench.py [--batch 64] [--reps 4] [--iters 10]
                                      [--out profiles/convnext_kernels.txt]
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

STAGES = {"tiny": [(56, 96), (28, 192), (14, 384), (7, 768)],
          "large": [(56, 192), (28, 384), (14, 768), (7, 1536)]}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--models", default="tiny,large")
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=10, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls per candidate")
    ap.add_argument("--drop", type=float, default=0.1, help="stochastic depth of scale_residual")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 4)

    import torch
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import _ref
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("convnext_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"convnext_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    bf = torch.bfloat16
    B, p, seed = a.batch, a.drop, 1234
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    shapes = []
    for name in a.models.split(","):
        for hw, c in STAGES[name]:
            if (hw, c) not in shapes:
                shapes.append((hw, c))
    with ClockSampler(0) as cs:
        for hw, C in shapes:
            torch.manual_seed(0)
            x = torch.randn(B, hw, hw, C, device="cuda").to(bf)
            dy = torch.randn(B, hw, hw, C, device="cuda").to(bf)
            add = torch.randn(B, hw, hw, C, device="cuda").to(bf)
            w = (torch.randn(C, 7, 7, 1, device="cuda") / 7).to(bf)
            bias = torch.randn(C, device="cuda")
            gamma = torch.rand(C, device="cuda")
            dw, db = torch.zeros(C, 1, 7, 7, device="cuda"), torch.zeros(C, device="cuda")
            dwg = torch.zeros(C, 7, 7, 1, device="cuda")
            dg, dlb = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            s = _ref._path_scale(x, hw * hw, p, seed).reshape(B, hw, hw, 1).contiguous()
            st, pd = (1, 1), (3, 3)

            def aten_sr_fwd():
                return (add.float() + (x.float() * gamma) * s).to(bf)

            def aten_sr_bwd():
                d = dy.float()
                df = ((d * gamma) * s).to(bf)
                dg.add_(((d * x.float()) * s).reshape(-1, C).sum(0))
                dlb.add_(df.reshape(-1, C).sum(0, dtype=torch.float32))
                return df

            act = x.numel() * 2
            cands = {
                "dwconv7_fwd/hip": (lambda: K.dwconv7_fwd(x, w, bias), 2 * act),
                "dwconv7_fwd/generic": (lambda: K.gconv_fwd(x, w, st, pd, C, bias), 2 * act),
                "dwconv7_dgrad/hip": (lambda: K.dwconv7_dgrad(dy, w, add), 3 * act),
                "dwconv7_dgrad/generic+add": (
                    lambda: K.gconv_dgrad(dy, w, x.shape, st, pd, C).add_(add), 3 * act),
                "dwconv7_wgrad/hip": (lambda: K.dwconv7_wgrad(dy, x, dw.reshape(-1), db), 2 * act),
                "dwconv7_wgrad/generic": (
                    lambda: K.gconv_wgrad(dy, x, 7, 7, st, pd, C, out=dwg, dbias=db), 2 * act),
                "scale_residual_fwd/hip": (
                    lambda: K.scale_residual_fwd(x, add, gamma, hw * hw, p, seed), 3 * act),
                "scale_residual_fwd/aten": (aten_sr_fwd, 3 * act),
                "scale_residual_bwd/hip": (
                    lambda: K.scale_residual_bwd(dy, x, gamma, hw * hw, p, seed, dg, dlb), 3 * act),
                "scale_residual_bwd/aten": (aten_sr_bwd, 3 * act),
            }
            for fn, _ in cands.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            us = {k: [] for k in cands}
            for _ in range(a.reps):
                for k, (fn, _) in cands.items():
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    us[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
            keys = list(cands)
            for i in range(0, len(keys), 2):
                k, ref = keys[i], keys[i + 1]
                for name in (k, ref):
                    med = statistics.median(us[name])
                    rec = {"shape": [B, hw, hw, C], "candidate": name, "us_per_call": round(med, 2),
                           "us_all": [round(v, 2) for v in us[name]],
                           "bytes_min": cands[name][1],
                           "TB_per_s": round(cands[name][1] / med / 1e6, 3)}
                    if name == k:
                        rec["vs"] = ref
                        rec["speedup"] = round(statistics.median(us[ref]) / med, 3)
                        rec["faster_in_every_alternation"] = all(
                            h < r for h, r in zip(us[k], us[ref]))
                    emit(rec)
    emit({"batch": B, "dtype": "bf16", "drop": p, "gpu_clocks": cs.summary(), "reps": a.reps,
          "iters": a.iters})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
