"""The ``eval_stats`` kernel against ``top1_correct`` and against the ATen composition that yields
the same quantities, and one ResNet-50 evaluation epoch with ``--eval-metrics top1`` against
``full``.

Kernel comparison, on ``[256, 1000]`` and ``[1024, 1000]`` logits, bf16 and fp32, in ONE process,
the candidates alternated ``--reps`` times (at least four), ``--iters`` calls between two device
events after ``--warmup`` untimed calls:

    top1_correct     the kernel evaluation uses today: one int32 count
    stats_counters   eval_stats, counters only (histogram and confusion pointers null)
    stats_hist       eval_stats, counters + confidence histogram
    stats_full       eval_stats, counters + histogram + confusion matrix: what EvalMeter launches
    aten             log_softmax + nll_loss(reduction='sum') + topk + argmax +
                     index_put_(accumulate=True), accumulated into device tensors without a sync

Per candidate it prints the mean and the median µs per call and every alternation.  No ratio is
fixed in advance: the batch is 0.5-4 MB and a launch is expected to be latency-bound.

Evaluation epoch: ResNet-50, batch 256 at 224x224, bf16, ``--batches`` batches held on the device,
``task.evaluate`` (top1) against ``task.evaluate_full`` (full), alternated ``--reps`` times.  The
one statement checked against the numbers (``epoch_within_bound``): the mean ``full`` epoch does
not exceed the mean ``top1`` epoch by more than the min-max spread of the ``top1`` alternations
plus batches x (stats_full - top1_correct) of the bf16 [256, 1000] kernel comparison.
``full_nocm`` is the same epoch with the confusion matrix off: the difference to ``full`` is the
per-evaluation cost of reading a 1000 x 1000 matrix back and deriving the per-class figures on the
host, which does not grow with the number of batches.

Usage: python tools/eval_stats_bench.py [--reps 4] [--iters 200] [--batches 4]
                                        [--out profiles/eval_stats.txt]
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

# hipcc -Rpass-analysis=kernel-resource-usage, gfx950 (csrc/kernels/eval_stats.hip's header)
KERNEL_RESOURCES = {
    "eval_stats_kernel<float,true>": {"vgprs": 25, "sgprs": 49, "scratch": 0, "lds_bytes": 192},
    "eval_stats_kernel<float,false>": {"vgprs": 25, "sgprs": 41, "scratch": 0, "lds_bytes": 192},
    "eval_stats_kernel<bf16,true>": {"vgprs": 25, "sgprs": 49, "scratch": 0, "lds_bytes": 192},
    "eval_stats_kernel<bf16,false>": {"vgprs": 25, "sgprs": 41, "scratch": 0, "lds_bytes": 192},
}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=200, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=20, help="untimed calls per candidate")
    ap.add_argument("--batches", type=int, default=4, help="batches of the evaluation epoch")
    ap.add_argument("--no-epoch", action="store_true", help="kernel comparison only")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 4)

    import torch
    import torch.nn.functional as F
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("eval_stats_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"eval_stats_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    emit({"kernel_resources": KERNEL_RESOURCES})
    per_batch_delta_us = None
    for dtype in (torch.bfloat16, torch.float32):
        for R in (256, 1024):
            V = 1000
            g = torch.Generator().manual_seed(R)
            logits = (torch.randn(R, V, generator=g) * 3).to(dtype).to(dev)
            labels = torch.randint(0, V, (R,), generator=g).to(dev)
            top1 = torch.zeros(1, dtype=torch.int32, device=dev)
            cnt = torch.zeros(8, dtype=torch.int64, device=dev)
            hist = torch.zeros(3, 15, dtype=torch.int64, device=dev)
            cm = torch.zeros(V, V, dtype=torch.int32, device=dev)
            acc = torch.zeros(3, dtype=torch.float64, device=dev)  # loss, top1, top5
            cm64 = torch.zeros(V, V, dtype=torch.int64, device=dev)
            ones = torch.ones(R, dtype=torch.int64, device=dev)

            def aten():
                lp = F.log_softmax(logits.float(), 1)
                acc[0] += F.nll_loss(lp, labels, reduction="sum")
                acc[2] += (logits.topk(5, 1).indices == labels[:, None]).any(1).sum()
                pred = logits.argmax(1)
                acc[1] += (pred == labels).sum()
                cm64.index_put_((labels, pred), ones, accumulate=True)

            cands = {
                "top1_correct": lambda: K.top1_correct(logits, labels, top1),
                "stats_counters": lambda: K.eval_stats(logits, labels, cnt, None, None, 5),
                "stats_hist": lambda: K.eval_stats(logits, labels, cnt, None, hist, 5),
                "stats_full": lambda: K.eval_stats(logits, labels, cnt, cm, hist, 5),
                "aten": aten,
            }
            for f in cands.values():
                for _ in range(a.warmup):
                    f()
            torch.cuda.synchronize()
            us = {m: [] for m in cands}
            for _ in range(a.reps):
                for m, f in cands.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        f()
                    e1.record()
                    e1.synchronize()
                    us[m].append(e0.elapsed_time(e1) * 1e3 / a.iters)
            name = str(dtype).replace("torch.", "")
            for m in cands:
                emit({"shape": [R, V], "dtype": name, "candidate": m,
                      "us_mean": round(statistics.mean(us[m]), 2),
                      "us_median": round(statistics.median(us[m]), 2),
                      "us_all": [round(v, 2) for v in us[m]],
                      "vs_top1_correct": round(statistics.mean(us[m])
                                               / statistics.mean(us["top1_correct"]), 3)})
            if dtype == torch.bfloat16 and R == 256:
                per_batch_delta_us = (statistics.mean(us["stats_full"])
                                      - statistics.mean(us["top1_correct"]))
    if not a.no_epoch:
        from mipipe.metrics import EvalMeter
        from mipipe.models import create_model
        from mipipe.train import task as T
        torch.manual_seed(0)
        model = create_model("resnet50", num_classes=1000)
        model.compute_dtype = torch.bfloat16
        model = model.to(dev).eval()
        g = torch.Generator().manual_seed(1)
        loader = [(torch.randn(256, 3, 224, 224, generator=g).to(dev),
                   torch.randint(0, 1000, (256,), generator=g).to(dev)) for _ in range(a.batches)]
        meter = EvalMeter(1000, topk=5, device=dev)
        meter_nocm = EvalMeter(1000, topk=5, confusion=False, device=dev)
        modes = {"top1": lambda: T.evaluate(model, dev, loader),
                 "full": lambda: T.evaluate_full(model, dev, loader, meter)["accuracy"],
                 "full_nocm": lambda: T.evaluate_full(model, dev, loader, meter_nocm)["accuracy"]}
        accs = {m: f() for m, f in modes.items()}  # warm-up: tuning, allocations
        for f in modes.values():
            f()
        ms = {m: [] for m in modes}
        for _ in range(a.reps):
            for m, f in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()  # ends with the host read of the result
                ms[m].append((time.perf_counter() - t0) * 1e3)
        mean = {m: statistics.mean(v) for m, v in ms.items()}
        spread = max(ms["top1"]) - min(ms["top1"])
        bound = spread + a.batches * per_batch_delta_us / 1e3
        emit({"epoch": "resnet50 b256 224x224 bf16", "batches": a.batches,
              "top1_ms_all": [round(v, 3) for v in ms["top1"]],
              "full_ms_all": [round(v, 3) for v in ms["full"]],
              "top1_ms_mean": round(mean["top1"], 3), "full_ms_mean": round(mean["full"], 3),
              "full_nocm_ms_all": [round(v, 3) for v in ms["full_nocm"]],
              "full_nocm_ms_mean": round(mean["full_nocm"], 3),
              "full_minus_top1_ms": round(mean["full"] - mean["top1"], 3),
              "full_nocm_minus_top1_ms": round(mean["full_nocm"] - mean["top1"], 3),
              "top1_spread_ms": round(spread, 3),
              "kernel_delta_us_per_batch": round(per_batch_delta_us, 2),
              "bound_ms": round(bound, 3),
              "epoch_within_bound": bool(mean["full"] - mean["top1"] <= bound),
              "same_accuracy": accs["top1"] == accs["full"] == accs["full_nocm"]})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
