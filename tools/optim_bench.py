"""Optimizer step alone, at real model sizes: SGD vs LARS and AdamW vs LAMB, with and without
global-norm clipping.

Builds the flat parameter space of the real model (ResNet-50: 25.6 M parameters, BERT-base:
110 M), fills the gradient buffer with random values and times ``optimizer.step()`` only.  All
modes run in ONE process on the same buffers, alternated ``--reps`` times (at least three); a
timed loop is ``--iters`` steps between two device events after ``--warmup`` untimed steps.  Per
mode it prints the median µs per step, the bytes the algorithm has to move per step, the TB/s that
gives, and the ratio to the plain optimizer of the same family next to the ratio of the bytes:

    sgd 22 B/param (reads p g m, writes p m + bf16 shadow)        lars 8 + 22 = 30
    adamw 30 B/param (reads p g m v, writes p m v + shadow)       lamb 24 + 18 = 42, clip +4

``--single MODE`` runs a few steps of one mode and nothing else — the program to put behind
``rocprofv3 --kernel-trace --stats --`` to see which launch holds the time.

Usage: python tools/optim_bench.py [--models resnet50,bert_base] [--reps 3] [--iters 50]
                                   [--out profiles/optim_large_batch.txt]
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

BYTES = {"sgd": 22, "lars": 30, "lars_clip": 30, "adamw": 30, "lamb": 42, "lamb_clip": 46}
PLAIN = {"lars": "sgd", "lars_clip": "sgd", "lamb": "adamw", "lamb_clip": "adamw"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="resnet50,bert_base")
    ap.add_argument("--reps", type=int, default=3, help="alternated repetitions per mode (>= 3)")
    ap.add_argument("--iters", type=int, default=50, help="steps per timed loop")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per mode")
    ap.add_argument("--single", choices=sorted(BYTES), default=None,
                    help="a few steps of this mode and nothing else (for a kernel trace)")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 3)

    import torch
    from mipipe.models import create_model
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops._native import load_error, native_available
    from mipipe.optim import LAMB, LARS, SGD, AdamW, LRSchedule

    if not torch.cuda.is_available():
        print("optim_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"optim_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    for name in a.models.split(","):
        torch.manual_seed(0)
        kw = {"num_classes": 1000} if name.startswith("resnet") else {}
        model = create_model(name, **kw).cuda()
        params = [p for p in model.parameters() if p.requires_grad]
        sched = LRSchedule("cosine", 1e-4, 10, 100000)
        # every optimizer works on the one flat space of these parameters, with its own state
        opts = {"sgd": SGD(params, 1e-4, momentum=0.9, weight_decay=1e-4),
                "adamw": AdamW(params, 1e-5, weight_decay=0.01),
                "lars": LARS(params, sched, momentum=0.9, weight_decay=1e-4),
                "lamb": LAMB(params, LRSchedule("cosine", 1e-5, 10, 100000), weight_decay=0.01)}
        space = opts["sgd"].space
        assert all(o.space is space for o in opts.values())
        space.flat_grad.normal_(0.0, 1e-2)
        for a0, b0, p in space.ranges():  # padding holds zeros, as after a real backward
            space.flat_grad[a0 + p.numel():b0].zero_()
        n = space.numel

        def run(mode, steps):
            o = opts[mode.split("_")[0]]
            if mode.startswith(("lars", "lamb")):
                o.param_groups[0]["max_grad_norm"] = 1.0 if mode.endswith("_clip") else None
            for _ in range(steps):
                o.step()

        if a.single is not None:
            run(a.single, 5)
            torch.cuda.synchronize()
            emit({"model": name, "single": a.single, "steps": 5, "flat_numel": n})
            continue

        modes = list(BYTES)
        for m in modes:
            run(m, a.warmup)
        torch.cuda.synchronize()
        us = {m: [] for m in modes}
        with ClockSampler(0) as cs:
            for _ in range(a.reps):
                for m in modes:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(m, a.iters)
                    e1.record()
                    e1.synchronize()
                    us[m].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        assert torch.isfinite(space.flat).all()
        med = {m: statistics.median(v) for m, v in us.items()}
        for m in modes:
            by = BYTES[m] * n
            rec = {"model": name, "mode": m, "flat_numel": n, "segments": len(space.order),
                   "us_per_step": round(med[m], 2), "us_all": [round(v, 2) for v in us[m]],
                   "bytes_per_step": by, "TB_per_s": round(by / med[m] / 1e6, 3)}
            if m in PLAIN:
                rec["vs_plain"] = round(med[m] / med[PLAIN[m]], 3)
                rec["bytes_vs_plain"] = round(BYTES[m] / BYTES[PLAIN[m]], 3)
            emit(rec)
        emit({"model": name, "gpu_clocks": cs.summary(), "reps": a.reps, "iters": a.iters})
        del opts, model, params, space
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
