"""Eval-mode forward throughput: the usual path against fused evaluation.

Runs ``model.eval()`` forwards under ``torch.no_grad()`` on one GPU with the switch of
``mipipe.ops.inference`` off and on, alternated ``--reps`` times (at least three) in the same
process on the same weights and batch.  A warm-up in each mode first lets benchmark mode pick
the conv plans (the fused convs are tuned under their own keys); every timed loop is ``--iters``
forwards between two ``torch.cuda.synchronize()``.  Prints one JSON line per measurement (ms per
forward, img/s) and a summary line with the medians, the largest output difference between the
modes and the GPU's clocks sampled during the run; ``--out`` also writes them to a file.

``--single off|on`` runs ONE forward in that mode and nothing else — the program to put behind
``rocprofv3 --kernel-trace --stats --`` for a per-kernel table of a single forward
(tools/kernel_stats.py); ``--save-table`` / ``--tune-table`` carry the plans picked by a full
run over to it, so the trace holds no tuning launches.

Usage: python tools/eval_bench.py [--arch resnet50] [--batch 256] [--image-size 224]
                                  [--dtype bf16] [--reps 3] [--out profiles/eval_fused_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--reps", type=int, default=3, help="alternated repetitions per mode (>= 3)")
    ap.add_argument("--iters", type=int, default=30, help="forwards per timed loop")
    ap.add_argument("--warmup", type=int, default=3, help="untimed forwards per mode")
    ap.add_argument("--num-classes", type=int, default=1000)
    ap.add_argument("--tune", type=int, choices=[0, 1], default=1,
                    help="benchmark mode: time the conv plans per shape in the warm-up")
    ap.add_argument("--tune-table", default="", help="load conv plans from this JSON file")
    ap.add_argument("--save-table", default="", help="write the plans in use to this JSON file")
    ap.add_argument("--single", choices=["off", "on"], default=None,
                    help="one forward in this mode and nothing else (for a kernel trace)")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 3)

    import torch
    from mipipe.models import create_model
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import tuning
    from mipipe.ops._native import load_error, native_available
    from mipipe.ops.inference import fused_eval

    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU (a CPU timing says nothing about the MI355X)")
    if not native_available():
        raise SystemExit(f"mipipe._C not loadable: {load_error()!r}")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    model = create_model(a.arch, num_classes=a.num_classes).to(dev).eval()
    model.compute_dtype = dt
    x = torch.randn(a.batch, 3, a.image_size, a.image_size, device=dev)
    if a.tune_table:
        tuning.load(a.tune_table)
    tuning.set_benchmark(bool(a.tune) and a.single is None)

    def forward(fused: bool):
        with torch.no_grad(), fused_eval(fused):
            return model(x)

    if a.single is not None:
        forward(a.single == "on")
        torch.cuda.synchronize()
        print(json.dumps({"single": a.single, "arch": a.arch, "batch": a.batch}), flush=True)
        return 0

    lines = []

    def emit(rec):
        s = json.dumps(rec)
        lines.append(s)
        print(s, flush=True)

    outs = {}
    for fused in (False, True):  # warm-up: code objects, plan tuning, allocator
        for _ in range(max(a.warmup, 1)):
            outs[fused] = forward(fused)
        torch.cuda.synchronize()
    o0, o1 = (outs[k].float().flatten() for k in (False, True))
    diff = {"max_abs_diff": float((o0 - o1).abs().max()), "out_abs_max": float(o0.abs().max()),
            "cosine": float(torch.nn.functional.cosine_similarity(o0, o1, dim=0))}
    if a.save_table:
        tuning.save(a.save_table)
    ms = {False: [], True: []}
    with ClockSampler(0) as cs:
        for rep in range(a.reps):
            for fused in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    forward(fused)
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e3 / a.iters
                ms[fused].append(t)
                emit({"rep": rep, "fused_eval": fused, "ms_per_forward": round(t, 4),
                      "img_per_s": round(a.batch / t * 1e3, 1)})
    med = {k: statistics.median(v) for k, v in ms.items()}
    emit({"summary": True, "arch": a.arch, "batch": a.batch, "image_size": a.image_size,
          "dtype": a.dtype, "reps": a.reps, "iters": a.iters, "tuned": bool(a.tune),
          "ms_off_median": round(med[False], 4), "ms_on_median": round(med[True], 4),
          "img_per_s_off": round(a.batch / med[False] * 1e3, 1),
          "img_per_s_on": round(a.batch / med[True] * 1e3, 1),
          "speedup_median": round(med[False] / med[True], 4),
          "fused_faster_in_every_rep": all(n < f for f, n in zip(ms[False], ms[True])),
          "outputs_off_vs_on": diff, "gpu_clocks": cs.summary()})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
