"""BASELINE config 5: a 3-step kfp.v2 pipeline  preprocess -> train -> eval (+ gated deploy).

The reference pipeline declares ``baseline_accuracy`` but never uses it (SURVEY.md §2.1 O6,
pytorch-pipeline.ipynb:218-221); its notebook placeholders (nb:10, nb:20) ask for a data step
before training.  This pipeline completes that design on one MI355X node:

1. ``preprocess`` writes the dataset as CIFAR-binary record files (synthetic & learnable: no
   network) into a ``Dataset`` artifact, with a manifest (stored shape, label width, class count,
   mean / std) that ``train`` and ``evaluate`` read;
2. ``train`` launches the distributed training job through the aiplatform-compatible job API
   (local launcher, one rank per GPU, RCCL DDP) running mipipe's task.py on those records via
   the native multi-threaded loader; the trained model lands in a ``Model`` artifact;
3. ``evaluate`` scores the model on the test records (HIP kernels on GPU), logs accuracy and a
   confusion matrix, and decides ``deploy`` against ``baseline_accuracy``;
4. ``deploy`` (inside ``dsl.Condition(deploy == "true")``) publishes the model to the serving
   directory.

Run (8 GPUs, ResNet-50 @ CIFAR shape):
  python examples/three_step_pipeline.py --gpus 8 --arch resnet50 --epochs 2
Run (8 GPUs, ResNet-50 @ ImageNet shape: 256x256 records, 1000 classes, 2-byte labels;
RandomResizedCrop(224) + flip for training and the 7/8 centre crop for evaluation, both decoded
on the GPU):
  python examples/three_step_pipeline.py --gpus 8 --arch resnet50 --dataset imagenet \
      --record-size 256 --image-size 224 --num-classes 1000 --epochs 2 \
      --extra-args '["--device-decode=1"]'
CPU smoke (config 1 style):
  python examples/three_step_pipeline.py --gpus 0 --arch mnist_cnn --dataset mnist --epochs 1
"""
import argparse
import json
import os
import sys
from typing import NamedTuple

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mipipe import kfp  # noqa: E402
from mipipe.dsl import (component, Input, Output, Dataset, Model, Metrics,  # noqa: E402
                        ClassificationMetrics)


@component()
def preprocess(dataset: str, n_train: int, n_test: int, seed: int, record_size: int,
               num_classes: int, label_bytes: int, data: Output[Dataset]):
    """``record_size`` (stored H = W), ``num_classes``, ``label_bytes``: 0 = the dataset's own
    (10 classes; 2-byte labels from 257 classes on)."""
    import json
    import os
    from mipipe.data import records as REC
    from mipipe.data.synthetic import DATASET_SHAPES
    ncls = num_classes or 10
    lb = label_bytes or (2 if ncls > 256 else 1)
    shape = (DATASET_SHAPES[dataset][0], record_size, record_size) if record_size else None
    man = REC.write_synthetic_dataset(data.path, dataset, n_train=n_train, n_test=n_test,
                                      seed=seed, num_classes=ncls, shape=shape, label_bytes=lb)
    mean, std = {"mnist": (REC.MNIST_MEAN, REC.MNIST_STD),
                 "imagenet": (REC.IMAGENET_MEAN, REC.IMAGENET_STD)}.get(
                     dataset, (REC.CIFAR10_MEAN, REC.CIFAR10_STD))
    man.update(mean=list(mean), std=list(std))
    data.metadata.update({k: v for k, v in man.items() if k != "files"})
    with open(os.path.join(data.path, "manifest.json"), "w") as f:
        json.dump(man, f)
    print(f"wrote {n_train}+{n_test} {dataset} records to {data.path}")


@component()
def train(data: Input[Dataset], arch: str, dataset: str, epochs: int, batch_size: int,
          gpus: int, learning_rate: float, extra_args: str, image_size: int,
          model: Output[Model], metrics: Output[Metrics]) -> float:
    import json
    import os
    from datetime import datetime
    from google.cloud import aiplatform
    from google.cloud.aiplatform import gapic as aip
    import mipipe.train.task as task_mod

    ts = datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
    aiplatform.init(project="local", location="local")
    args = ["--dist-url=env://", f"--arch={arch}", f"--dataset={dataset}",
            f"--data-dir={data.path}", f"--num_epochs={epochs}", f"--batch_size={batch_size}",
            f"--learning_rate={learning_rate}", "--eval-every=1000", "--log-every=10",
            "--model_filename=model.pth", f"--num_classes={int(data.metadata.get('num_classes', 10))}"
            ] + ([f"--image-size={image_size}"] if image_size else []) + json.loads(extra_args)
    if gpus > 1:
        args.append("--multiprocessing-distributed")
    job = aiplatform.CustomTrainingJob(display_name=f"train_{arch}_{ts}",
                                       script_path=task_mod.__file__, container_uri="local")
    accel = aip.AcceleratorType.AMD_INSTINCT_MI355X if gpus else None
    job.run(args=args, replica_count=1, machine_type="local",
            accelerator_type=accel.name if accel else None, accelerator_count=gpus,
            base_output_dir=model.path)
    acc, found = 0.0, False
    for root, _, files in os.walk(model.path):
        for fn in files:
            if fn.endswith(".log"):
                with open(os.path.join(root, fn)) as f:
                    for line in f:
                        if "MIPIPE_METRICS" in line:
                            m = json.loads(line.split("MIPIPE_METRICS", 1)[1])
                            found = True
                            acc = float(m["accuracy"])
                            for k, v in m.items():
                                if isinstance(v, (int, float)):
                                    metrics.log_metric(k, v)
    if not found:
        raise RuntimeError("training job produced no metrics line")
    model.metadata.update({"arch": arch, "dataset": dataset, "framework": "mipipe",
                           "image_size": image_size})
    return acc * 100.0


@component()
def evaluate(data: Input[Dataset], model: Input[Model], arch: str, dataset: str,
             baseline_accuracy: float, metrics: Output[ClassificationMetrics],
             summary: Output[Metrics]) -> NamedTuple("EvalOutput", [("accuracy", float),
                                                                     ("deploy", str)]):
    import os
    from collections import namedtuple
    import json
    import torch
    from mipipe.data import records as REC
    from mipipe.data.synthetic import DATASET_SHAPES
    from mipipe.models import create_model
    from mipipe.train.checkpoint import strip_module_prefix

    path = None
    for root, _, files in os.walk(model.path):
        for fn in files:
            if fn == "model.pth":
                path = os.path.join(root, fn)
    if path is None:
        raise FileNotFoundError(f"no model.pth under {model.path}")
    # stored shape, label width and mean / std: the manifest preprocess wrote, else the metadata
    man = dict(data.metadata)
    mpath = os.path.join(data.path, "manifest.json")
    if os.path.isfile(mpath):
        with open(mpath) as f:
            man.update(json.load(f))
    shape = tuple(int(v) for v in man.get("shape", DATASET_SHAPES[dataset][:3]))
    size = int(model.metadata.get("image_size", 0)) or DATASET_SHAPES[dataset][1]
    sd = strip_module_prefix(torch.load(path, map_location="cpu", weights_only=True))
    head = [v for k, v in sd.items() if v.dim() == 2][-1]  # classifier weight [classes, feat]
    ncls = int(head.shape[0])
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    kw = ({"in_chans": shape[0]}
          if arch == "mnist_cnn" or arch.startswith(("resnet", "wide_resnet", "resnext")) else {})
    net = create_model(arch, num_classes=ncls, **kw)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    mean, std = ((REC.MNIST_MEAN, REC.MNIST_STD) if dataset == "mnist"
                 else (REC.CIFAR10_MEAN, REC.CIFAR10_STD))
    if "mean" in man and "std" in man:
        mean, std = tuple(man["mean"]), tuple(man["std"])
    files = REC.dataset_files(data.path, dataset, "test")
    # stored size != model size: the rrc evaluation transform (7/8 centre crop, resized)
    rkw = ({"transform": "rrc", "out_size": (size, size)} if shape[1:] != (size, size) else {})
    loader = REC.RecordDataLoader(files, shape, 256, train=False, mean=mean, std=std,
                                  device=dev, label_bytes=int(man.get("label_bytes", 1)),
                                  decode="device" if dev.type == "cuda" and rkw else "host",
                                  **rkw)
    from mipipe.metrics import EvalMeter
    meter = EvalMeter(ncls, device=dev)  # one eval_stats launch per batch, one read at the end
    with torch.no_grad():
        for x, y in loader:
            meter.update(net(x), y)
    res = meter.log_to(metrics)  # confusion matrix + confidenceMetrics
    hits = sum(row[i] for i, row in enumerate(res["confusion"]))
    acc = 100.0 * float(hits) / max(1, res["rows"])
    summary.log_metric("accuracy", acc)
    summary.log_metric("loss", res["loss"])
    summary.log_metric(f"accuracy_top{meter.topk}", 100.0 * res[f"accuracy_top{meter.topk}"])
    summary.log_metric("ece", res["ece"])
    summary.log_metric("baseline_accuracy", baseline_accuracy)
    deploy = "true" if acc >= baseline_accuracy else "false"
    summary.log_metric("deploy", 1.0 if deploy == "true" else 0.0)
    print(f"test accuracy {acc:.2f}% vs baseline {baseline_accuracy}% -> deploy={deploy}")
    out = namedtuple("EvalOutput", ["accuracy", "deploy"])
    return out(acc, deploy)


@component()
def deploy(model: Input[Model], serving_dir: str) -> str:
    import os
    import shutil
    dst = os.path.join(serving_dir, os.path.basename(model.path.rstrip("/")))
    shutil.copytree(model.path, dst, dirs_exist_ok=True)
    print(f"deployed {model.path} -> {dst}")
    return dst


@kfp.dsl.pipeline(name="preprocess-train-eval")
def pipeline(baseline_accuracy: float = 70.0, dataset: str = "cifar10", arch: str = "resnet50",
             n_train: int = 10000, n_test: int = 2000, epochs: int = 2, batch_size: int = 256,
             gpus: int = 8, learning_rate: float = 0.1, extra_args: str = "[]",
             serving_dir: str = "/tmp/mipipe_serving", seed: int = 0, record_size: int = 0,
             image_size: int = 0, num_classes: int = 0, label_bytes: int = 0):
    pre = preprocess(dataset, n_train, n_test, seed, record_size, num_classes, label_bytes)
    tr = train(pre.outputs["data"], arch, dataset, epochs, batch_size, gpus, learning_rate,
               extra_args, image_size)
    ev = evaluate(pre.outputs["data"], tr.outputs["model"], arch, dataset, baseline_accuracy)
    with kfp.dsl.Condition(ev.outputs["deploy"] == "true"):
        deploy(tr.outputs["model"], serving_dir)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=8)
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--dataset", default="cifar10")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--n-train", type=int, default=10000)
    ap.add_argument("--n-test", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--baseline-accuracy", type=float, default=70.0)
    ap.add_argument("--extra-args", default="[]")
    ap.add_argument("--serving-dir", default="/tmp/mipipe_serving")
    ap.add_argument("--record-size", type=int, default=0,
                    help="stored H = W of the records (0: the dataset's own shape)")
    ap.add_argument("--image-size", type=int, default=0,
                    help="model input H = W (0: the dataset's own); differs from the stored "
                         "size -> RandomResizedCrop / centre-crop records (the rrc transform)")
    ap.add_argument("--num-classes", type=int, default=0,
                    help="classes of the synthetic set (0: 10); above 256 the labels take 2 bytes")
    ap.add_argument("--spec", default="three_step.json")
    ap.add_argument("--pipeline-root", default="gs://mipipe/pipeline_root")
    a = ap.parse_args(argv)
    from mipipe.kfp.v2 import compiler
    from mipipe.kfp.v2.google.client import AIPlatformClient
    compiler.Compiler().compile(pipeline_func=pipeline, package_path=a.spec)
    client = AIPlatformClient(project_id="local", region="local")
    resp = client.create_run_from_job_spec(
        a.spec, pipeline_root=a.pipeline_root,
        parameter_values={"baseline_accuracy": a.baseline_accuracy, "dataset": a.dataset,
                          "arch": a.arch, "n_train": a.n_train, "n_test": a.n_test,
                          "epochs": a.epochs, "batch_size": a.batch_size, "gpus": a.gpus,
                          "learning_rate": a.lr, "extra_args": a.extra_args,
                          "serving_dir": a.serving_dir, "record_size": a.record_size,
                          "image_size": a.image_size, "num_classes": a.num_classes}, sync=True)
    run = client.get_run(resp["runId"])
    print(json.dumps({"run": resp["runId"], "state": run["state"],
                      "tasks": {k: v.get("state") for k, v in run.get("tasks", {}).items()}}))
    return 0 if run["state"] == "PIPELINE_STATE_SUCCEEDED" else 1


if __name__ == "__main__":
    sys.exit(main())
