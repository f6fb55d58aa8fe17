"""Weight-EMA kernels alone, at real flat-buffer sizes: ``ema_update`` against ATen's ``lerp_``,
``ema_swap``, a skipped (``every``) call and a whole ``ModelEMA.update()``; and the training step
with and without the EMA (``--task-ab``).

Builds the flat parameter space of the real model (ResNet-50: 25.6 M parameters, BERT-base:
109.5 M) and times, in ONE process on one GPU, alternated ``--reps`` times (at least four),
``--iters`` calls between two device events after ``--warmup`` untimed calls:

    hip_update         K.ema_update: reads p and e, writes e — 12 B/parameter (streaming accesses,
                       the default policy of the optimizer state)
    hip_update_cached  the same with the streaming bit of ``set_nt_store`` cleared for the loop
    aten_lerp          ema.lerp_(flat, w) with a host weight: the same bytes
    hip_swap           K.ema_swap: reads p and e, writes p, e and the bf16 shadow — 18 B/parameter
    hip_skip           K.ema_update on a call the device counter skips: no bytes
    ema_object         ModelEMA.update(): counter add + hip_update + the buffer kernel

In a training step neither p nor the average is in the 256 MB memory-side cache when the update
starts (19 ms of activation traffic lie between two updates).  The candidates above therefore
rotate over enough (p, e) buffer pairs that at least 512 MB of other pairs pass between two uses of
one: "cold".  ``*_warm`` are the same calls on ONE pair back to back, where a working set below
256 MB (ResNet-50: 204 MB) stays in that cache — a state no training step sees, recorded for
completeness.

Per candidate it prints the median µs per call, the spread of the alternations
((max − min) / median), the bytes that must move and the TB/s that gives.  The acceptance
condition — ``hip_update`` not slower than ``aten_lerp`` by more than the spread of the
alternations of the two — is decided on the cold measurement (``not_slower_beyond_spread``).

``--task-ab N``: instead, run ``python -m mipipe.train.task`` ResNet-50 b256 ``--hip-graph
--steps 35 --warmup-steps 5`` N times without and N times with ``--model-ema-decay 0.9999``,
alternated, one process each, and print ms per step = 256000 / ``samples_per_sec_per_rank`` of
each run's metrics file (30 measured steps).

Usage: python tools/ema_bench.py [--models resnet50,bert_base] [--reps 4] [--iters 48]
                                 [--out profiles/model_ema.txt]
       python tools/ema_bench.py --task-ab 3
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

BYTES = {"hip_update": 12, "hip_update_cached": 12, "aten_lerp": 12, "hip_swap": 18, "hip_skip": 0,
         "ema_object": 12, "hip_update_warm": 12, "hip_update_cached_warm": 12, "aten_lerp_warm": 12}
COLD_GAP_BYTES = 512 << 20  # bytes of other pairs between two uses of one pair: twice the cache

TASK_ARGS = ["--arch", "resnet50", "--dataset", "imagenet", "--batch_size", "256", "--num_epochs",
             "1", "--steps", "35", "--warmup-steps", "5", "--hip-graph", "--train-samples", "8960",
             "--test-samples", "256", "--log-every", "0", "--local_training"]


def task_ab(n: int, out: str) -> int:
    """off / ema alternated n times, one process each; ms per step from each run's metrics."""
    import subprocess
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(1, n + 1):
            for kind, extra in (("off", []), ("ema", ["--model-ema-decay", "0.9999"])):
                mf = os.path.join(tmp, f"{kind}{i}.json")
                cmd = [sys.executable, "-m", "mipipe.train.task"] + TASK_ARGS + [
                    "--model_dir", os.path.join(tmp, "model"), "--metrics-file", mf] + extra
                r = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                   text=True)
                if r.returncode != 0:
                    print(r.stdout[-2000:], file=sys.stderr)
                    return r.returncode
                with open(mf) as f:
                    m = json.load(f)
                sps = m["samples_per_sec_per_rank"]
                line = (f"AB {kind} {i} img/s {sps:.1f} ms/step {256e3 / sps:.3f} loss {m['loss']} "
                        f"graph {m['hip_graph']} ema_updates {m.get('ema_updates')}")
                print(line, flush=True)
                lines.append(line)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", default="resnet50,bert_base")
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=48, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=8, help="untimed calls per candidate")
    ap.add_argument("--task-ab", type=int, default=0, metavar="N",
                    help="the ResNet-50 step without / with the EMA, alternated N times")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if a.task_ab:
        return task_ab(a.task_ab, a.out)
    a.reps = max(a.reps, 4)

    import torch
    from mipipe.models import create_model
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native, native_available
    from mipipe.optim import SGD, ModelEMA

    if not torch.cuda.is_available():
        print("ema_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"ema_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2
    C = native()
    nt_mask = C.get_nt_store()

    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    for name in a.models.split(","):
        torch.manual_seed(0)
        kw = {"num_classes": 1000} if name.startswith("resnet") else {}
        model = create_model(name, **kw).cuda()
        opt = SGD([p for p in model.parameters() if p.requires_grad], 1e-4, momentum=0.9)
        space = opt.space
        ema = ModelEMA(model, decay=0.9999, every=1, warmup=True)
        ema.update()  # settles the buffer table
        n = space.numel
        w = 1.0 - 0.9999
        one = torch.ones(1, dtype=torch.int32, device="cuda")  # call 1: averages when every = 1
        scal = torch.zeros(4, dtype=torch.float32, device="cuda")
        npairs = 1 + -(-COLD_GAP_BYTES // (8 * n))
        pairs = [(space.flat.clone(), space.flat.clone()) for _ in range(npairs)]
        a.iters = -(-a.iters // (2 * npairs)) * 2 * npairs  # whole rotations, an even number of swaps
        a.warmup = -(-a.warmup // (2 * npairs)) * 2 * npairs

        def rot(fn, k):  # call number i works on pair i mod k
            def loop(calls):
                for i in range(calls):
                    fn(*pairs[i % k])
            return loop

        def cached(loop):  # the streaming bit of the optimizer state cleared for this loop
            def run(calls):
                C.set_nt_store(nt_mask & ~1024)
                try:
                    loop(calls)
                finally:
                    C.set_nt_store(nt_mask)
            return run

        def upd(p, e):
            K.ema_update(p, e, one, 1, w, False, scal)

        def lerp(p, e):
            e.lerp_(p, w)

        cands = {
            "hip_update": rot(upd, npairs),
            "hip_update_cached": cached(rot(upd, npairs)),
            "aten_lerp": rot(lerp, npairs),
            "hip_swap": rot(lambda p, e: K.ema_swap(p, e, space.shadow), npairs),
            "hip_skip": rot(lambda p, e: K.ema_update(p, e, one, 2, w, False, scal), npairs),
            "ema_object": lambda calls: [ema.update() for _ in range(calls)],
            "hip_update_warm": rot(upd, 1),
            "hip_update_cached_warm": cached(rot(upd, 1)),
            "aten_lerp_warm": rot(lerp, 1),
        }
        for f in cands.values():
            f(a.warmup)
        torch.cuda.synchronize()
        us = {m: [] for m in cands}
        with ClockSampler(0) as cs:
            for _ in range(a.reps):
                for m, f in cands.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f(a.iters)
                    e1.record()
                    e1.synchronize()
                    us[m].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        assert torch.isfinite(space.flat).all() and torch.isfinite(ema.ema).all()
        assert all(torch.isfinite(e).all() for _, e in pairs)
        med = {m: statistics.median(v) for m, v in us.items()}
        spread = {m: (max(v) - min(v)) / med[m] for m, v in us.items()}
        for m in cands:
            by = BYTES[m] * n
            rec = {"model": name, "candidate": m, "flat_numel": n,
                   "pairs": 1 if m.endswith("_warm") or m == "ema_object" else npairs,
                   "us_per_call": round(med[m], 2), "us_all": [round(v, 2) for v in us[m]],
                   "spread": round(spread[m], 4), "bytes_min": by,
                   "TB_per_s": round(by / med[m] / 1e6, 3)}
            if m.startswith("hip_update"):
                ref = "aten_lerp_warm" if m.endswith("_warm") else "aten_lerp"
                tol = max(spread[m], spread[ref])
                rec.update(vs=ref, ratio=round(med[m] / med[ref], 4), spread_of_pair=round(tol, 4))
                if m == "hip_update":  # the acceptance condition: the default path, cold
                    rec["not_slower_beyond_spread"] = bool(med[m] <= med[ref] * (1 + tol))
            emit(rec)
        emit({"model": name, "ema_buffer_elems": int(ema._nbuf), "gpu_clocks": cs.summary(),
              "reps": a.reps, "iters": a.iters, "nt_store_mask": nt_mask})
        del cands, pairs, ema, opt, model, space
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
