"""``batch_mix`` alone at the ImageNet batch shape, against the ATen compositions a user would write.

At ``[256, 3, 224, 224]`` (``--shape``) in bf16 and fp32, Mixup and CutMix at lambda = 0.5 (CutMix:
the centred 158 x 158 box, ``int(224 * sqrt(0.5))``):

    mixup   hip_inplace, hip_out        vs  aten: x.mul(lam).add_(x.flip(0), alpha=1 - lam)
    cutmix  hip_inplace                 vs  aten_inplace: x[box] = x.flip(0)[box]
            hip_out                     vs  aten_out:     y = x.clone(); y[box] = x.flip(0)[box]

All candidates run in ONE process on the same buffers, alternated ``--reps`` times (at least
four); a timed loop is ``--iters`` calls between two device events after ``--warmup`` untimed
calls, and the shader clock is sampled meanwhile (mipipe/obs/clocks.py).  Per candidate it prints
the µs per call of every alternation, the median, the bytes the operation has to move (each
element it touches read once and written once) and the TB/s that gives; per comparison whether the
kernel was faster in EVERY alternation.

``--single NAME`` runs a few calls of one candidate and nothing else (for a kernel trace).

Usage: python tools/mix_bench.py [--reps 4] [--iters 20] [--out profiles/batch_mix.txt]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# candidate -> the ATen comparator of the same operation
VERSUS = {"mixup/hip_inplace": "mixup/aten", "mixup/hip_out": "mixup/aten",
          "cutmix/hip_inplace": "cutmix/aten_inplace", "cutmix/hip_out": "cutmix/aten_out"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", default="256,3,224,224")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls per candidate")
    ap.add_argument("--single", default=None, help="a few calls of this candidate only")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 4)

    import torch
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("mix_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"mix_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    B, C, H, W = (int(v) for v in a.shape.split(","))
    lam = 0.5
    ch, cw = int(H * math.sqrt(1 - lam)), int(W * math.sqrt(1 - lam))
    y0, x0 = (H - ch) // 2, (W - cw) // 2
    y1, x1 = y0 + ch, x0 + cw
    box_frac = ch * cw / float(H * W)
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    for dname in a.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
        torch.manual_seed(0)
        x = torch.randn(B, C, H, W, device="cuda").to(dtype)
        out = torch.empty_like(x)
        mixup = torch.tensor([lam, 1, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
        cutmix = torch.tensor([1 - box_frac, 2, y0, y1, x0, x1, 0, 0], dtype=torch.float32,
                              device="cuda")
        full = 2 * x.numel() * x.element_size()  # every element read once, written once

        def aten_cut_inplace():
            x[:, :, y0:y1, x0:x1] = x.flip(0)[:, :, y0:y1, x0:x1]

        def aten_cut_out():
            y = x.clone()
            y[:, :, y0:y1, x0:x1] = x.flip(0)[:, :, y0:y1, x0:x1]
            return y

        cands = {
            "mixup/hip_inplace": (lambda: K.batch_mix(x, mixup, out=x), full),
            "mixup/hip_out": (lambda: K.batch_mix(x, mixup, out=out), full),
            "mixup/aten": (lambda: x.mul(lam).add_(x.flip(0), alpha=1 - lam), full),
            "cutmix/hip_inplace": (lambda: K.batch_mix(x, cutmix, out=x), int(full * box_frac)),
            "cutmix/hip_out": (lambda: K.batch_mix(x, cutmix, out=out), full),
            "cutmix/aten_inplace": (aten_cut_inplace, int(full * box_frac)),
            "cutmix/aten_out": (aten_cut_out, full),
        }
        if a.single is not None:
            for _ in range(5):
                cands[a.single][0]()
            torch.cuda.synchronize()
            emit({"dtype": dname, "single": a.single, "calls": 5})
            continue
        for fn, _ in cands.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in cands}
        with ClockSampler(0) as cs:
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
        assert torch.isfinite(x.float()).all()
        for k, (_, by) in cands.items():
            med = statistics.median(us[k])
            rec = {"shape": [B, C, H, W], "dtype": dname, "candidate": k,
                   "us_per_call": round(med, 2), "us_all": [round(v, 2) for v in us[k]],
                   "bytes_min": by, "TB_per_s": round(by / med / 1e6, 3)}
            if k in VERSUS:
                ref = us[VERSUS[k]]
                rec["vs"] = VERSUS[k]
                rec["speedup"] = round(statistics.median(ref) / med, 3)
                rec["faster_in_every_alternation"] = all(h < r for h, r in zip(us[k], ref))
            emit(rec)
        emit({"dtype": dname, "box": [y0, y1, x0, x1], "box_fraction": round(box_frac, 4),
              "gpu_clocks": cs.summary(), "reps": a.reps, "iters": a.iters})
        del x, out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
