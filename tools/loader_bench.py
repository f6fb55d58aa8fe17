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

Usage: python tools/loader_bench.py [--n 51200] [--batch 1024] [--workers 8] [--reps 3]
                                    [--out profiles/loader_bench.txt]
       python tools/loader_bench.py --transform rrc --record-size 256 --image-size 224 \
                                    --n 2048 --batch 256 --dtype bf16
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
    loaders = {m: R.RecordDataLoader(files, shape, a.batch, train=True, seed=0, workers=a.workers,
                                     prefetch=a.prefetch, device=dev, decode=m,
                                     out_dtype=out_dtype, **kw)
               for m in ("host", "device")}
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


if __name__ == "__main__":
    sys.exit(main())
