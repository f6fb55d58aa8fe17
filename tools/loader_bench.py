"""Record-loader throughput: ``decode="host"`` against ``decode="device"``.

Times whole epochs of a synthetic CIFAR-shape record set (3x32x32, 3073-byte records) at batch
1024 on one GPU, (a) through the loader alone — every batch is brought to the device, nothing
consumes it — and (b) through a ResNet-18 fp32 training step per batch.  The two decode modes
run in the same process on the same files, alternated ``--reps`` times; each timed loop ends in
``torch.cuda.synchronize()``, lasts at least ``--min-seconds`` (epochs repeat until then) and
excludes its warm-up iterations.  Prints one JSON line per measurement and a summary line (median
img/s per mode and the GPU's clocks sampled during the run); ``--out`` also writes them to a file.

``--transform rrc --record-size S --image-size R`` measures the resizing transform instead
(SxS records with 2-byte labels, RandomResizedCrop to RxR; ``--dtype bf16`` for bf16 batches):
the loader alone by default, ``--train-step 1`` adds the ResNet-18 loop.

``--auto-augment ta_wide`` / ``--random-erase P`` turn the per-sample augmentation on in both
loaders.  ``--augment-sweep`` instead alternates three variants of the ``decode="device"`` loader
in one process — off, ``ta_wide``, ``ta_wide`` + erase (``--random-erase``, default 0.1) —
``--reps`` times, then times ``record_augment`` (one block per sample, and split by size) and
``batch_erase_`` alone (and ``record_augment`` with one op of each code path pinned for the whole
batch) on one uploaded batch with device events (``--kernel-calls N`` launches
each; 0 skips it; ``--kernels-only`` runs nothing else, for a profiler run).

Usage: python tools/loader_bench.py [--n 51200] [--batch 1024] [--workers 8] [--reps 3]
                                    [--out profiles/loader_bench.txt]
       python tools/loader_bench.py --transform rrc --record-size 256 --image-size 224 \
                                    --n 2048 --batch 256 --dtype bf16
       python tools/loader_bench.py --transform rrc --record-size 256 --image-size 224 \
                                    --n 2048 --batch 256 --dtype bf16 --augment-sweep --reps 4
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=51200, help="records in the set (one epoch)")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--prefetch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3, help="alternated repetitions per mode")
    ap.add_argument("--warmup", type=int, default=5, help="untimed batches / steps per loop")
    ap.add_argument("--min-seconds", type=float, default=1.5,
                    help="a measurement repeats whole epochs until this much time has passed")
    ap.add_argument("--transform", choices=["crop", "rrc"], default="crop")
    ap.add_argument("--record-size", type=int, default=256, help="rrc: stored H = W")
    ap.add_argument("--image-size", type=int, default=224, help="rrc: output H = W")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32", help="batch dtype")
    ap.add_argument("--train-step", type=int, choices=[0, 1], default=None,
                    help="also time a ResNet-18 training step per batch (default: crop only)")
    ap.add_argument("--auto-augment", choices=["none", "ta_wide"], default="none")
    ap.add_argument("--random-erase", type=float, default=None, metavar="P")
    ap.add_argument("--augment-sweep", action="store_true",
                    help="alternate off / ta_wide / ta_wide + erase on the device-decode loader")
    ap.add_argument("--kernel-calls", type=int, default=50,
                    help="--augment-sweep: launches per kernel timed alone (0: skip)")
    ap.add_argument("--kernels-only", action="store_true",
                    help="--augment-sweep: only the kernels-alone part")
    ap.add_argument("--data-dir", default="", help="reuse / keep the record files here")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)

    import torch
    from mipipe.data import records as R
    from mipipe.models import create_model
    from mipipe.ops._native import load_error, native_available
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops.functional import cross_entropy
    from mipipe.optim import SGD
    from mipipe.runtime import runtime_available
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench needs a GPU")
    if not native_available():
        raise SystemExit(f"mipipe._C not loadable: {load_error()!r}")
    if not runtime_available():
        raise SystemExit("mipipe._runtime is not built")
    dev = torch.device("cuda", 0)

    tmp = None
    data_dir = a.data_dir
    if not data_dir:
        tmp = tempfile.TemporaryDirectory(prefix="loader_bench_")
        data_dir = tmp.name
    rrc = a.transform == "rrc"
    name = "imagenet" if rrc else "cifar10"
    shape = (3, a.record_size, a.record_size) if rrc else (3, 32, 32)
    out_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    train_step = bool(a.train_step) if a.train_step is not None else not rrc
    files = R.dataset_files(data_dir, name, "train")
    if not files:
        R.write_synthetic_dataset(data_dir, name, n_train=a.n, n_test=16, seed=0, shape=shape,
                                  num_classes=1000 if rrc else 10, label_bytes=2 if rrc else 1)
        files = R.dataset_files(data_dir, name, "train")

    kw = (dict(transform="rrc", out_size=(a.image_size, a.image_size), label_bytes=2,
               mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD) if rrc else dict(pad=4))
    def make(mode, **extra):
        return R.RecordDataLoader(files, shape, a.batch, train=True, seed=0, workers=a.workers,
                                  prefetch=a.prefetch, device=dev, decode=mode,
                                  out_dtype=out_dtype, **kw, **extra)

    if a.augment_sweep:
        return _augment_sweep(a, make, dev, shape, out_dtype, torch, ClockSampler)
    akw = {}
    if a.auto_augment != "none" or a.random_erase:
        akw = dict(auto_augment=a.auto_augment, random_erase=a.random_erase or 0.0)
    loaders = {m: make(m, **akw) for m in ("host", "device")}
    n_total = loaders["host"].num_samples_total

    torch.manual_seed(0)
    model = create_model("resnet18", num_classes=1000 if rrc else 10, in_chans=3).to(dev)
    model.compute_dtype = out_dtype
    opt = SGD(model.parameters(), 0.1, momentum=0.9, weight_decay=1e-4)
    model.train()

    def step(x, y):
        opt.zero_grad()
        loss = cross_entropy(model(x), y)
        loss.backward()
        opt.step()

    def run(mode: str, train: bool, epoch: int):
        """(img/s, next epoch): whole epochs until --min-seconds have passed, the first
        epoch's warm-up batches excluded."""
        dl = loaders[mode]
        seen = 0
        t0 = None
        while True:
            dl.set_epoch(epoch)
            epoch += 1
            for k, (x, y) in enumerate(dl):
                if t0 is None and k == a.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if train:
                    step(x, y)
                if t0 is not None:
                    seen += x.shape[0]
            torch.cuda.synchronize()
            if t0 is None:
                raise SystemExit("--n is too small for --warmup")
            dt = time.perf_counter() - t0
            if dt >= a.min_seconds:
                return seen / dt, epoch

    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    res = {(m, t): [] for m in loaders for t in (False, True)}
    epoch = 0
    with ClockSampler(dev.index or 0) as cs:
        for train in ((False, True) if train_step else (False,)):
            for rep in range(a.reps):
                for mode in ("host", "device"):
                    v, epoch = run(mode, train, epoch)
                    res[(mode, train)].append(v)
                    emit({"what": f"resnet18_{a.dtype}_step" if train else "loader_alone",
                          "decode": mode, "rep": rep, "img_per_s": round(v, 1)})
    med = {f"{'train' if t else 'loader'}_{m}": round(statistics.median(v), 1)
           for (m, t), v in res.items() if v}
    emit({"summary": med, "transform": a.transform, "record_shape": list(shape),
          "out_size": [a.image_size] * 2 if rrc else list(shape[1:]), "dtype": a.dtype,
          "records": n_total, "batch": a.batch, "workers": a.workers,
          "auto_augment": a.auto_augment, "random_erase": a.random_erase or 0.0,
          "prefetch": a.prefetch, "warmup_batches": a.warmup, "reps": a.reps,
          "host_cpus": len(os.sched_getaffinity(0)), "gpu": torch.cuda.get_device_name(0),
          "min_seconds": a.min_seconds, "gpu_clocks": cs.summary(),
          "loader_speedup": round(med["loader_device"] / med["loader_host"], 2),
          **({"train_speedup": round(med["train_device"] / med["train_host"], 2)}
             if train_step else {})})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    del loaders
    if tmp is not None:
        tmp.cleanup()
    return 0


def _augment_sweep(a, make, dev, shape, out_dtype, torch, ClockSampler) -> int:
    """off / ta_wide / ta_wide + erase on the device-decode loader, alternated; then the two
    kernels alone."""
    from mipipe.data.records import augment_force, erase_pq
    from mipipe.ops import kernels as K
    from mipipe.ops._native import native
    p = 0.1 if a.random_erase is None else a.random_erase
    variants = {"off": {}, "ta_wide": dict(auto_augment="ta_wide"),
                f"ta_wide+erase{p:g}": dict(auto_augment="ta_wide", random_erase=p)}
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def run(dl, epoch):
        seen, t0 = 0, None
        while True:
            dl.set_epoch(epoch)
            epoch += 1
            for k, (x, _) in enumerate(dl):
                if t0 is None and k == a.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                if t0 is not None:
                    seen += x.shape[0]
            torch.cuda.synchronize()
            if t0 is None:
                raise SystemExit("--n is too small for --warmup")
            dt = time.perf_counter() - t0
            if dt >= a.min_seconds:
                return seen / dt, epoch

    with ClockSampler(dev.index or 0) as cs:
        res = {v: [] for v in variants}
        if not a.kernels_only:
            loaders = {v: make("device", **kw) for v, kw in variants.items()}
            epoch = 0
            for rep in range(a.reps):
                for v, dl in loaders.items():
                    r, epoch = run(dl, epoch)
                    res[v].append(r)
                    emit({"what": "loader_alone", "decode": "device", "augment": v, "rep": rep,
                          "img_per_s": round(r, 1)})
            del loaders
        kern = {}
        if a.kernel_calls > 0:
            dl = make("device")
            dl.set_epoch(0)
            rs, gs = dl._stage[0]
            dl._ld.start_epoch(list(iter(dl.sampler)), 0)
            n = dl._ld.next_raw_into(rs.data_ptr(), gs.data_ptr())
            rec, gi = rs[:n].to(dev), gs[:n].to(dev)
            Ho = Wo = a.image_size if a.transform == "rrc" else shape[1]
            x = torch.randn(n, shape[0], Ho, Wo, device=dev).to(out_dtype)
            lb = dl.label_bytes
            auto = native().record_augment_parts(*shape)
            calls = {"record_augment/parts=1": lambda: K.record_augment(rec, gi, shape, 0, 0, lb,
                                                                        parts=1),
                     f"record_augment/parts={auto}": lambda: K.record_augment(rec, gi, shape, 0,
                                                                              0, lb),
                     **{f"record_augment/{op}": (lambda f=augment_force(op, 15, 1):
                                                 K.record_augment(rec, gi, shape, 0, 0, lb, force=f))
                        for op in ("Identity", "Solarize", "Contrast", "Equalize", "Color",
                                   "Sharpness", "Rotate")},
                     f"batch_erase_/p={p:g}": lambda: K.batch_erase_(x, gi, 0, 0, erase_pq(p)),
                     "batch_erase_/p=1": lambda: K.batch_erase_(x, gi, 0, 0, 1 << 24)}
            for rep in range(max(1, min(a.reps, 4))):
                for name, fn in calls.items():
                    for _ in range(5):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.kernel_calls):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us = e0.elapsed_time(e1) * 1000.0 / a.kernel_calls
                    kern.setdefault(name, []).append(us)
                    emit({"what": "kernel_alone", "kernel": name, "rep": rep, "batch": n,
                          "calls": a.kernel_calls, "us_per_launch": round(us, 1)})
    emit({"summary": {v: round(statistics.median(r), 1) for v, r in res.items() if r},
          "spread": {v: [round(min(r), 1), round(max(r), 1)] for v, r in res.items() if r},
          "kernel_us_median": {k: round(statistics.median(v), 1) for k, v in kern.items()},
          "transform": a.transform, "record_shape": list(shape), "image_size": a.image_size,
          "dtype": a.dtype, "batch": a.batch, "workers": a.workers, "prefetch": a.prefetch,
          "warmup_batches": a.warmup, "reps": a.reps, "min_seconds": a.min_seconds,
          "gpu": torch.cuda.get_device_name(0), "gpu_clocks": cs.summary()})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
