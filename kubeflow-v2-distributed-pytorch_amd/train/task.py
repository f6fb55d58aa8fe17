"""Distributed training entry point — flag-compatible with the reference's ``task.py``.

Reference: /root/reference/task.py (318 lines).  Same CLI flags with the same names and
defaults (task.py:55-95) so the compiled pipeline's args
(``--dist-url=env:// --multiprocessing-distributed --num_epochs=2``, nb:159-163) work
unchanged, the same env contract (``WORLD_SIZE``/``RANK``/``MASTER_*``/``AIP_MODEL_DIR``) and
the same process structure: ``main()`` resolves the distributed mode (task.py:97-113) and
either ``mp.spawn``s one worker per local GPU (task.py:117-124) or runs ``main_worker``
in-process (task.py:127); ``main_worker`` does rank math + rendezvous (task.py:132-150),
seeding (161-162), model construction (165-171), DDP wrapping (173-208), loss/optimizer
(210-214), resume (216-242), data (246-267), the epoch loop with periodic eval + export
(272-312).

Deliberate fixes of reference quirks, each noted inline:
  * evaluation runs on the *unwrapped* model, sharded over all ranks (no rank-0-only
    collective mismatch, §5.2); the model is also evaluated and saved after training;
  * ``--resume`` takes a path (or ``auto``) and ``start_epoch`` is honoured;
  * ``DistributedSampler.set_epoch`` is called; ``--dist-url`` defaults to ``env://``;
  * per-process batch = ``--batch_size`` (what the reference effectively does), reported
    together with the global batch;
  * data is synthetic and generated on the GPU (no download race, no CPU decode).
Additions: ``--dtype``, ``--dataset``, ``--steps``, ``--bench``, ``--num_classes``,
``--eval-every``, metrics JSON with samples/sec, fault injection for tests.

Large-batch training (``mipipe.optim.LARS`` / ``LAMB``; all of it stays on under ``--hip-graph``,
the per-step values being device memory):
  * ``--optimizer {sgd,lars,lamb,adamw}`` (default ``sgd``: the reference's SGD, unchanged);
    ``adamw`` is the flat-buffer ``mipipe.optim.AdamW`` at a constant ``--learning_rate`` with
    ``--wd`` (the ViT recipe's optimizer; schedules, warm-up and clipping live in ``lamb``);
  * ``--lr-schedule {constant,linear,poly,cosine}`` with ``--lr-warmup-steps`` and
    ``--lr-total-steps`` (default ``num_epochs`` x steps per epoch): linear warm-up to
    ``--learning_rate``, then the decay to 0;
  * ``--clip-grad-norm N``: global-norm gradient clipping;
  * ``--trust-coefficient`` (default 0.001): LARS's trust coefficient.
``--optimizer sgd`` with a schedule or clipping runs ``LARS(trust_coefficient=None)``: the same
update as SGD with a device-side learning rate.  With a schedule active the step log line and
``metrics.json`` carry ``lr``.

Regularisers (all off by default; :mod:`mipipe.data.mix`):
  * ``--label-smoothing EPS``: the loss kernels' label smoothing;
  * ``--mixup-alpha A`` / ``--cutmix-alpha A`` with ``--mix-prob`` and ``--mix-switch-prob``:
    timm's batch-mode Mixup / CutMix.  Each training step builds its descriptor from
    ``(random_seed, rank, epoch, step)``, mixes the batch with its own reverse in one kernel
    (``batch_mix``) and takes the pair-target loss (``cross_entropy_mixed``); both read the
    descriptor on the device, so the step stays capturable (``--hip-graph``: the descriptor is the
    captured step's third input).  Evaluation is never mixed.  The step log line and
    ``metrics.json`` carry ``mix_mode`` and ``mix_lambda``.

Per-sample augmentation of record data (off by default; needs ``--data-dir``):
  * ``--auto-augment ta_wide``: TrivialAugmentWide, one of 14 ops per image at one of 31
    magnitudes; ``--random-erase P``: Random Erasing with probability ``P``.  The order is augment
    -> crop / rrc -> erase: the augmentation acts on the stored image, before the crop
    (torchvision augments after it), the erase on the normalised batch.  Both are functions of
    ``(random_seed, epoch, sample index)``, the same bits with ``--device-decode`` 0 and 1 (the
    ``record_augment`` and ``batch_erase`` kernels); evaluation is never augmented.  The start-up
    line and ``metrics.json`` carry ``auto_augment`` and ``random_erase``.

Weight averaging (off by default; :class:`mipipe.optim.ModelEMA`):
  * ``--model-ema-decay D`` (0 = off) with ``--model-ema-steps N`` (average every N-th step) and
    ``--model-ema-warmup {0,1}`` (timm's ``min(D, (1+u)/(10+u))`` warm-up).  ``D`` is used as
    given: torchvision's adjustment by batch size and epochs is the caller's to make.  The update
    follows ``optimizer.step()`` and reads its call count on the device, so it is captured under
    ``--hip-graph``.  Every evaluation runs twice, on the live model and with the average swapped
    in place under the model: the printed line and ``metrics.json`` gain ``accuracy_ema`` and
    ``ema_updates``, the export a second file ``<stem>_ema<ext>``, the checkpoint ``model_ema``.
    ``--resume`` restores the average together with its call count and its decay / steps / warmup:
    the checkpoint's settings replace the command line's (a line is printed when they differ).

Evaluation metrics (:class:`mipipe.metrics.EvalMeter`, one ``eval_stats`` launch per batch):
  * ``--eval-metrics {top1,full}`` (default ``top1``: the evaluation and the metrics as before).
    ``full`` adds top-k accuracy (``--eval-topk K``, default 5), the validation loss, the expected
    calibration error and, up to 4096 classes, the confusion matrix with macro-F1 and balanced
    accuracy: the ``Accuracy:`` line gains the top-k accuracy and the loss, ``metrics.json`` gains
    ``accuracy_top{k}``, ``eval_loss``, ``ece``, ``macro_f1`` and ``balanced_accuracy`` (with a
    weight EMA the same keys suffixed ``_ema``).  ``accuracy`` is the same float in both modes.
  * ``--eval-report PATH``: rank 0 writes the full result dict (confusion matrix, per-class
    figures, confidence curve) of the last evaluation there.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time
from datetime import datetime

if __package__ in (None, ""):  # executed as a plain script (the pipeline stages it as task.py)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch
import torch.multiprocessing as mp

from mipipe.models import create_model, model_names
from mipipe.obs import trace
from mipipe.obs.log import JsonlLogger
from mipipe.launch.env import device_offset, local_gpus
from mipipe.parallel import DataParallel, DistributedDataParallel, DistributedSampler
from mipipe.parallel import dist_utils
from mipipe.data.synthetic import DATASET_SHAPES, DeviceBatchLoader, SyntheticImageDataset
from mipipe.optim import SGD, AdamW
from mipipe.ops import functional as MF
from mipipe.ops import inference
from mipipe.train import checkpoint as ckpt
from mipipe.obs.meter import ThroughputMeter

best_acc1 = 0.0


def _make_optimizer(args, params, shadow_dtype):
    """The run's optimizer.  The default flags give the reference's SGD (task.py:212-214) exactly
    as before; a schedule, a warm-up or clipping with ``--optimizer sgd`` gives the same update
    rule as ``LARS(trust_coefficient=None)``, whose learning rate lives on the device."""
    plain = (args.lr_schedule == "constant" and args.lr_warmup_steps == 0
             and args.clip_grad_norm is None)
    if args.optimizer == "sgd" and plain:
        return SGD(params, args.learning_rate, momentum=args.momentum,
                   weight_decay=args.weight_decay, shadow_dtype=shadow_dtype)
    if args.optimizer == "adamw":
        if not plain:
            raise SystemExit("--optimizer adamw runs at a constant learning rate without "
                             "clipping: for --lr-schedule / --lr-warmup-steps / --clip-grad-norm "
                             "use --optimizer lamb, which keeps them on the device")
        return AdamW(params, args.learning_rate, weight_decay=args.weight_decay,
                     shadow_dtype=shadow_dtype)
    from mipipe.optim import LAMB, LARS, LRSchedule
    sched = LRSchedule(args.lr_schedule, args.learning_rate, args.lr_warmup_steps,
                       args.lr_total_steps or 0)
    if args.optimizer == "lamb":
        return LAMB(params, sched, weight_decay=args.weight_decay,
                    max_grad_norm=args.clip_grad_norm, shadow_dtype=shadow_dtype)
    lars = args.optimizer == "lars"
    # sgd: decay on every parameter, as the reference's SGD has it
    return LARS(params, sched, momentum=args.momentum, weight_decay=args.weight_decay,
                trust_coefficient=args.trust_coefficient if lars else None,
                max_grad_norm=args.clip_grad_norm, exclude_1d=lars, shadow_dtype=shadow_dtype)


def set_random_seeds(random_seed: int = 0) -> None:
    """task.py:22-28: seed torch / numpy / random.  The reference's
    ``cudnn.deterministic = True`` maps to mipipe's deterministic mode (``--deterministic``,
    see :func:`configure_kernels`)."""
    torch.manual_seed(random_seed)
    np.random.seed(random_seed)
    random.seed(random_seed)


def configure_kernels(use_gpu: bool, deterministic: bool = True) -> None:
    """task.py:25-26 ``cudnn.deterministic = True`` -> mipipe's deterministic mode (fixed-order
    reductions, no float atomics: :mod:`mipipe.ops.determinism`); task.py:244
    ``cudnn.benchmark = True`` -> per-shape tile autotuning of the conv kernels
    (:mod:`mipipe.ops.tuning`; ``MIPIPE_BENCHMARK=0`` disables it, ``MIPIPE_TUNE_TABLE=path``
    starts from a saved table).  In deterministic mode nothing is picked by timing (the plan
    fixes the reduction order): a loaded / shipped table or the heuristic decides."""
    if not use_gpu:
        return
    from mipipe.ops import determinism, tuning
    determinism.set_deterministic(deterministic)
    tuning.from_env(deterministic)  # deterministic: shipped measured tables replace timing
    tuning.set_benchmark(os.environ.get("MIPIPE_BENCHMARK", "1") != "0",
                         verbose=os.environ.get("MIPIPE_TUNE_VERBOSE", "0") == "1")


class CrossEntropyLoss(torch.nn.Module):
    """``nn.CrossEntropyLoss()`` (task.py:211) on the fused log-softmax+NLL kernel."""

    def __init__(self, label_smoothing: float = 0.0, ignore_index: int = -100):
        super().__init__()
        self.label_smoothing = label_smoothing
        self.ignore_index = ignore_index

    def _ce(self, logits, labels, mix=None):
        if mix is not None:  # pair targets (Mixup / CutMix): every row counts, no ignore_index
            return MF.cross_entropy_mixed(logits, labels, mix, self.label_smoothing)
        return MF.cross_entropy(logits, labels, self.label_smoothing, self.ignore_index)

    def forward(self, logits, labels, mix=None):
        if isinstance(logits, tuple) and hasattr(logits, "_fields"):
            # GoogLeNet / Inception-v3 in training mode return torchvision's named tuples
            # (main logits + auxiliary classifiers).  The reference hands them to
            # nn.CrossEntropyLoss (task.py:310) and crashes; here the auxiliary losses are added
            # with the papers' weights: 0.3 per GoogLeNet head, 0.4 for Inception-v3's.
            w = 0.4 if len(logits) == 2 else 0.3
            loss = self._ce(logits[0], labels, mix)
            for aux in logits[1:]:
                if aux is not None:
                    loss = loss + w * self._ce(aux, labels, mix)
            return loss
        return self._ce(logits, labels, mix)


def _unwrap(model):
    return model.module if isinstance(model, (DistributedDataParallel, DataParallel,
                                          torch.nn.DataParallel)) else model


@torch.no_grad()
def evaluate(model, device, test_loader) -> float:
    """Top-1 accuracy (task.py:30-46) — argmax + correct count run in ONE fused kernel per
    batch (``top1_correct``, accumulating into a device counter) and the host reads one value
    at the end instead of a ``.item()`` per batch.  Sharded over ranks (each rank's loader
    holds its shard) and summed with one all-reduce."""
    from mipipe.ops import kernels as K
    m = _unwrap(model)
    was_training = m.training
    m.eval()
    correct = torch.zeros(1, dtype=torch.int32, device=device)
    total = 0
    for images, labels in test_loader:
        images, labels = images.to(device), labels.to(device)
        outputs = m(images)
        K.top1_correct(outputs, labels, correct)
        total += labels.numel()
    t = torch.stack([correct[0].to(torch.int64), torch.tensor(total, device=device)])
    if dist_utils.get_world_size() > 1:
        torch.distributed.all_reduce(t)
    if was_training:
        m.train()
    return float(t[0].item()) / max(1, int(t[1].item()))


@torch.no_grad()
def evaluate_full(model, device, test_loader, meter) -> dict:
    """:func:`evaluate` with every metric of ``meter`` (:class:`mipipe.metrics.EvalMeter`): one
    ``eval_stats`` launch per batch, sharded over ranks like :func:`evaluate`, summed with one
    all-reduce and read back once.  Returns the meter's result dict; ``accuracy`` is the float
    :func:`evaluate` returns."""
    m = _unwrap(model)
    was_training = m.training
    m.eval()
    meter.reset()
    for images, labels in test_loader:
        images, labels = images.to(device), labels.to(device)
        meter.update(m(images), labels)
    meter.all_reduce()
    if was_training:
        m.train()
    return meter.result()


# the keys of an EvalMeter result that --eval-metrics full adds to the run's metrics
def _full_metrics(res: dict, topk: int, suffix: str = "") -> dict:
    out = {f"accuracy_top{topk}{suffix}": res[f"accuracy_top{topk}"],
           f"eval_loss{suffix}": res["loss"], f"ece{suffix}": res["ece"]}
    for key in ("macro_f1", "balanced_accuracy"):
        if key in res:
            out[key + suffix] = res[key]
    return out


def build_parser() -> argparse.ArgumentParser:
    names = model_names()
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="mipipe distributed trainer (task.py compatible)")
    # --- reference flags (task.py:56-94), same names and defaults -------------------------
    p.add_argument("--local_rank", type=int, help="Local rank (torch.distributed.launch compat).")
    p.add_argument("--num_epochs", type=int, default=100, help="Number of training epochs.")
    p.add_argument("--batch_size", type=int, default=1024, help="Training batch size for one process.")
    p.add_argument("--learning_rate", dest="learning_rate", type=float, default=0.1, help="Learning rate.")
    p.add_argument("--random_seed", type=int, default=0, help="Random seed.")
    p.add_argument("--model_dir", type=str, default=os.environ.get("AIP_MODEL_DIR", ""),
                   help="Directory (or gs:// URI) for saving models.")
    p.add_argument("--model_filename", type=str, default="resnet_distributed.pth", help="Model filename.")
    p.add_argument("-a", "--arch", metavar="ARCH", default="resnet18", choices=names,
                   help="model architecture: " + " | ".join(names) + " (default: resnet18)")
    p.add_argument("--momentum", default=0.9, type=float, metavar="M", help="momentum")
    p.add_argument("--wd", "--weight-decay", default=1e-4, type=float, metavar="W",
                   dest="weight_decay", help="weight decay (default: 1e-4)")
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "lars", "lamb", "adamw"],
                   help="sgd (default), lars (vision, large batch), lamb (transformers, large "
                        "batch) or adamw (constant learning rate, --wd)")
    p.add_argument("--lr-schedule", default="constant",
                   choices=["constant", "linear", "poly", "cosine"],
                   help="learning-rate decay after the warm-up, evaluated on the device")
    p.add_argument("--lr-warmup-steps", type=int, default=0, help="linear warm-up steps")
    p.add_argument("--lr-total-steps", type=int, default=None,
                   help="steps until the schedule ends (default: num_epochs x steps per epoch)")
    p.add_argument("--clip-grad-norm", type=float, default=None,
                   help="clip the global gradient norm to this value")
    p.add_argument("--trust-coefficient", type=float, default=0.001,
                   help="LARS trust coefficient")
    p.add_argument("--label-smoothing", type=float, default=0.0,
                   help="label smoothing of the training loss")
    p.add_argument("--stochastic-depth", type=float, default=None, metavar="P",
                   help="stochastic depth of the convnext_* models (default: the family's own "
                        "value, e.g. 0.1 for convnext_tiny)")
    p.add_argument("--mixup-alpha", type=float, default=0.0,
                   help="Mixup: lambda ~ Beta(a, a); 0 = off")
    p.add_argument("--cutmix-alpha", type=float, default=0.0,
                   help="CutMix: box area from lambda ~ Beta(a, a); 0 = off")
    p.add_argument("--mix-prob", type=float, default=1.0,
                   help="probability that a training step is mixed at all")
    p.add_argument("--mix-switch-prob", type=float, default=0.5,
                   help="probability of CutMix when both alphas are set")
    p.add_argument("--model-ema-decay", type=float, default=0.0,
                   help="decay of the exponential moving average of the weights, used as given "
                        "(no batch-size adjustment); 0 = off. With --resume the checkpoint's "
                        "decay / steps / warmup replace these flags")
    p.add_argument("--model-ema-steps", type=int, default=1,
                   help="average every N-th training step")
    p.add_argument("--model-ema-warmup", type=int, choices=[0, 1], default=1,
                   help="1: decay min(D, (1+u)/(10+u)) at averaging update u (timm's warm-up)")
    p.add_argument("--pretrained", dest="pretrained", action="store_true",
                   help="use pre-trained model: torchvision-format weights from "
                        "--pretrained-weights or the torchvision cache (no network download)")
    p.add_argument("--pretrained-weights", dest="pretrained_weights", default=None,
                   help="path of a torchvision-format state_dict (.pth) for --pretrained")
    p.add_argument("--local_training", dest="local_training", action="store_true",
                   help="save to --model_dir instead of AIP_MODEL_DIR")
    p.add_argument("--rank", default=-1, type=int, help="node rank for distributed training")
    p.add_argument("--resume", nargs="?", const="auto", default="",
                   help="resume from checkpoint PATH ('auto' = <model_dir>/checkpoint.pth.tar)")
    p.add_argument("--world-size", default=int(os.getenv("WORLD_SIZE", -1)), type=int,
                   help="number of nodes for distributed training")
    p.add_argument("--dist-url", default="env://", type=str,
                   help="url used to set up distributed training (reference default "
                        "http://localhost:8082 is not a valid init method)")
    p.add_argument("--dist-backend", default="nccl", type=str,
                   help="distributed backend (nccl = RCCL on ROCm; gloo on CPU)")
    p.add_argument("--multiprocessing-distributed", action="store_true",
                   help="launch one process per local GPU (N per node)")
    p.add_argument("--gpu", default=None, type=int, help="GPU id to use.")
    p.add_argument("--workers", default=4, type=int, metavar="N",
                   help="data loading workers (data is generated on the device; kept for compat)")
    # --- additions ------------------------------------------------------------------------
    p.add_argument("--dataset", default="cifar10", choices=sorted(DATASET_SHAPES),
                   help="synthetic dataset shape")
    p.add_argument("--image-size", type=int, default=None, help="override image H=W")
    p.add_argument("--data-dir", default="",
                   help="directory with CIFAR-binary record files (<dataset>_{train,test}.bin or "
                        "cifar-10-batches-bin/); read by the native loader. Empty: synthetic "
                        "on-device data")
    p.add_argument("--device-decode", type=int, choices=[0, 1], default=0,
                   help="with --data-dir: 1 uploads the uint8 records and crops / flips / "
                        "normalises them on the device (same bits as the host loader's output)")
    p.add_argument("--record-transform", choices=["crop", "rrc"], default=None,
                   help="with --data-dir: crop = RandomCrop(padding) + flip at the stored size; "
                        "rrc = RandomResizedCrop + flip (7/8 centre crop for evaluation) resized "
                        "to the model's input size. Default: crop, or rrc when the data "
                        "directory's manifest.json stores another size than the model takes")
    p.add_argument("--auto-augment", choices=["none", "ta_wide"], default="none",
                   help="with --data-dir: ta_wide = TrivialAugmentWide on every training image "
                        "(one random op of 14 at a random magnitude), applied to the stored image "
                        "before the crop; on the device with --device-decode 1")
    p.add_argument("--random-erase", type=float, default=0.0, metavar="P",
                   help="with --data-dir: Random Erasing of the normalised training batch with "
                        "probability P (scale 0.02-0.33, ratio 0.3-3.3, value 0)")
    p.add_argument("--train-samples", type=int, default=None)
    p.add_argument("--test-samples", type=int, default=None)
    p.add_argument("--num_classes", type=int, default=None,
                   help="classifier width (reference keeps torchvision's 1000)")
    p.add_argument("--deterministic", dest="deterministic", action="store_true", default=True,
                   help="fixed-order reductions, bit-reproducible runs (reference task.py:25-26 "
                        "sets cudnn.deterministic); default on")
    p.add_argument("--no-deterministic", dest="deterministic", action="store_false",
                   help="allow float-atomic reductions (faster)")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"],
                   help="compute dtype on GPU (master weights stay fp32); CPU runs fp32")
    p.add_argument("--fused-eval", type=int, choices=[0, 1], default=0,
                   help="evaluate with BatchNorm, residual and ReLU fused into the conv epilogues "
                        "(mipipe.ops.inference; MIPIPE_FUSED_EVAL=1 turns it on as well)")
    p.add_argument("--eval-metrics", choices=["top1", "full"], default="top1",
                   help="top1: accuracy only; full: also top-k accuracy, loss, calibration error "
                        "and (up to 4096 classes) the confusion matrix, from one kernel per batch")
    p.add_argument("--eval-topk", type=int, default=5, help="k of the top-k accuracy (full)")
    p.add_argument("--eval-report", default="",
                   help="with --eval-metrics full: write the full result dict, confusion matrix "
                        "included, to this JSON file (rank 0)")
    p.add_argument("--hip-graph", action="store_true",
                   help="replay full-size training steps (forward, backward with the DDP bucket "
                        "all-reduces, SGD) from one captured hipGraph; partial batches run eagerly")
    p.add_argument("--steps", type=int, default=0, help="max training steps per epoch (0 = all)")
    p.add_argument("--eval-every", type=int, default=10, help="evaluate every N epochs (task.py:279)")
    p.add_argument("--log-every", type=int, default=20)
    p.add_argument("--warmup-steps", type=int, default=2, help="steps excluded from samples/sec")
    p.add_argument("--bucket-cap-mb", type=float, default=32.0)
    p.add_argument("--no-broadcast-buffers", action="store_true")
    p.add_argument("--dist-timeout", type=float, default=1800.0, help="collective timeout (s)")
    p.add_argument("--compat-nested-model-dir", action="store_true",
                   help="export to AIP_MODEL_DIR/model/<file> like task.py:291")
    p.add_argument("--metrics-file", default="", help="write final metrics JSON here")
    p.add_argument("--trace", action="store_true",
                   help="roctx ranges around step phases (for rocprofv3 --marker-trace)")
    p.add_argument("--log-dir", default=os.environ.get("MIPIPE_LOG_DIR", ""),
                   help="per-rank JSON-lines logs (rank<k>.jsonl)")
    p.add_argument("--cpu-procs", type=int, default=1,
                   help="processes per node when no GPU is visible (gloo)")
    return p


def _read_manifest(data_dir: str):
    """The dict of ``<data_dir>/manifest.json`` (shape, label_bytes, num_classes, ...) or None."""
    path = os.path.join(data_dir, "manifest.json") if data_dir else ""
    if not path or not os.path.isfile(path):
        return None
    with open(path) as f:
        man = json.load(f)
    if len(man.get("shape", ())) != 3:
        raise ValueError(f"{path}: 'shape' must be [C, H, W]")
    return man


def _ngpus() -> int:
    """GPUs of this node (replica): the launcher's MIPIPE_LOCAL_GPUS when it set one
    (launch/env.py), else every visible device."""
    if os.environ.get("MIPIPE_FORCE_CPU") == "1":
        return 0
    n = local_gpus()
    return n if n is not None else torch.cuda.device_count()


def main(argv=None) -> int:
    argv = build_parser().parse_args(argv)
    if argv.dist_url == "env://" and argv.world_size == -1:
        argv.world_size = int(os.environ.get("WORLD_SIZE", 1))
    argv.distributed = argv.world_size > 1 or argv.multiprocessing_distributed
    ngpus_per_node = _ngpus()
    procs_per_node = ngpus_per_node if ngpus_per_node > 0 else argv.cpu_procs
    if ngpus_per_node == 0:
        argv.dist_backend = "gloo"
    # debugging (task.py:104-113)
    print(f"os WORLD_SIZE={os.getenv('WORLD_SIZE', -1)}")
    print(f"os RANK={os.getenv('RANK', 0)}")
    print(f"os MASTER_ADDR={os.getenv('MASTER_ADDR', 'localhost')}")
    print(f"os MASTER_PORT={os.getenv('MASTER_PORT', '8082')}")
    print(f"Arg - distributed={argv.distributed}")
    print(f"Arg - multiprocessing_distributed={argv.multiprocessing_distributed}")
    print(f"Arg - dist_backend={argv.dist_backend}")
    print(f"Arg - dist_url={argv.dist_url}")
    print(f"ngpus_per_node={ngpus_per_node}")
    start = datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
    print(f"Starting training: {start}", flush=True)
    if argv.multiprocessing_distributed:
        argv.world_size = procs_per_node * argv.world_size  # task.py:120
        print(f"GPU x WORLD SIZE = {argv.world_size}")
        mp.spawn(main_worker, nprocs=procs_per_node, args=(procs_per_node, argv))
    else:
        main_worker(argv.gpu, procs_per_node, argv)
    end = datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
    print(f"Training complete: {end}", flush=True)
    return 0


def _fault_check(rank: int, step: int) -> None:
    spec = os.environ.get("MIPIPE_FAULT_INJECT")  # "rank:step[:code]"
    if not spec:
        return
    parts = spec.split(":")
    if int(parts[0]) == rank and int(parts[1]) == step:
        code = int(parts[2]) if len(parts) > 2 else 17
        print(f"[fault-injection] rank {rank} exiting with {code} at step {step}", flush=True)
        sys.stdout.flush()
        os._exit(code)


def main_worker(gpu, ngpus_per_node, args) -> dict:
    global best_acc1
    args.gpu = gpu
    if args.gpu is not None:
        print(f"Use GPU: {args.gpu} for training")
    if args.distributed:
        if args.dist_url == "env://" and args.rank == -1:
            args.rank = int(os.environ.get("RANK", 0))
            print(f"Distributed and getting rank from os.environ: rank={args.rank}")
        if args.multiprocessing_distributed:
            args.rank = dist_utils.global_rank(args.rank, ngpus_per_node, gpu)  # task.py:146
            print(f"Distributed and Multiprocesing. Setting rank for each worker. rank={args.rank}")
    else:
        args.rank = 0
    use_gpu = _ngpus() > 0
    if use_gpu:
        local = args.gpu if args.gpu is not None else int(os.environ.get("LOCAL_RANK", 0))
        local += device_offset()  # this replica's first GPU (launch/env.py)
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    else:
        device = torch.device("cpu")
    if args.distributed:
        dist_utils.init_distributed(args.dist_backend, args.dist_url, args.world_size, args.rank,
                                    args.dist_timeout, device if use_gpu else None)
        print("Process group initialized", flush=True)
    world = dist_utils.get_world_size()
    set_random_seeds(args.random_seed)  # same seed on every rank -> identical init (task.py:161)
    # cudnn.deterministic (task.py:25-26) / cudnn.benchmark (task.py:244) analogues
    configure_kernels(use_gpu, args.deterministic)

    if not 0.0 <= args.random_erase <= 1.0:
        raise SystemExit(f"--random-erase must be a probability in [0, 1], got {args.random_erase}")
    augmenting = args.auto_augment != "none" or args.random_erase > 0
    if augmenting and not args.data_dir:
        raise SystemExit("--auto-augment / --random-erase act on record data: they need "
                         "--data-dir (synthetic on-device data is not augmented)")
    if args.pretrained:
        print(f"=> using pre-trained model '{args.arch}'")  # task.py:167
    else:
        print(f"=> creating model '{args.arch}'")
    C, H, W, K, N = DATASET_SHAPES[args.dataset]
    if args.image_size:
        H = W = args.image_size
    # records: a manifest.json next to them (the pipeline's preprocess step writes one) carries
    # the stored shape, the label width and the class count; explicit flags win
    manifest = _read_manifest(args.data_dir)
    stored, label_bytes = (C, H, W), 1
    if manifest is not None:
        stored = tuple(int(v) for v in manifest["shape"])
        label_bytes = int(manifest.get("label_bytes", 1))
        C = stored[0]
        if args.num_classes is None and "num_classes" in manifest:
            args.num_classes = int(manifest["num_classes"])
    record_transform = args.record_transform or ("rrc" if stored[1:] != (H, W) else "crop")
    if record_transform == "crop":
        H, W = stored[1:]  # the crop transform keeps the stored size
    kw = {}
    if args.num_classes is not None:
        kw["num_classes"] = args.num_classes
    if args.arch == "mnist_cnn":
        kw.setdefault("num_classes", K)
        kw["in_chans"] = C
    elif args.arch.startswith(("resnet", "wide_resnet", "resnext")):
        kw["in_chans"] = C
    elif args.arch.startswith("vit_"):
        # the position table is built for one image size (no interpolation)
        if H != W:
            raise SystemExit(f"--arch {args.arch} needs square images, got {H}x{W}")
        kw["in_chans"] = C
        kw["image_size"] = H
    stochastic_depth = None
    if args.arch.startswith("convnext_"):
        if H % 4 or W % 4 or min(H, W) < 32:
            raise SystemExit(f"--arch {args.arch} needs images of at least 32x32 whose sides are "
                             f"multiples of 4, got {H}x{W}")
        if args.stochastic_depth is not None and not 0.0 <= args.stochastic_depth < 1.0:
            raise SystemExit(f"--stochastic-depth must be in [0, 1), got {args.stochastic_depth}")
        kw["in_chans"] = C
        kw["stochastic_depth_prob"] = args.stochastic_depth
        kw["seed"] = args.random_seed
    elif args.stochastic_depth is not None:
        raise SystemExit(f"--stochastic-depth applies to the convnext_* models only, not to "
                         f"--arch {args.arch}")
    model = create_model(args.arch, **kw)
    if args.arch.startswith("convnext_"):
        stochastic_depth = model.stochastic_depth_prob
        print(f"=> {args.arch}: stochastic depth {stochastic_depth:g}", flush=True)
    if args.pretrained:
        from mipipe.models import find_pretrained, load_pretrained
        wpath = find_pretrained(args.arch, args.pretrained_weights)
        if wpath is None:
            print(f"=> no local pre-trained weights for '{args.arch}' (no network access to "
                  "download them): random init")
        else:
            load_pretrained(model, wpath)
            print(f"=> loaded pre-trained weights from {wpath}")
    compute_dtype = torch.bfloat16 if (use_gpu and args.dtype == "bf16") else torch.float32
    if hasattr(model, "compute_dtype"):
        model.compute_dtype = compute_dtype
    model = model.to(device)
    if args.distributed:
        model = DistributedDataParallel(model, device_ids=[device.index] if use_gpu else None,
                                        bucket_cap_mb=args.bucket_cap_mb,
                                        broadcast_buffers=not args.no_broadcast_buffers)
    elif use_gpu and args.gpu is None and _ngpus() > 1:
        model = DataParallel(model)  # task.py:201-208 path (d), on this replica's GPUs
    criterion = CrossEntropyLoss(label_smoothing=args.label_smoothing).to(device)
    mixer = None
    if args.mixup_alpha > 0 or args.cutmix_alpha > 0:
        from mipipe.data.mix import BatchMixer
        from mipipe.ops import kernels as MK
        mixer = BatchMixer(args.random_seed, args.rank, device, mixup_alpha=args.mixup_alpha,
                           cutmix_alpha=args.cutmix_alpha, prob=args.mix_prob,
                           switch_prob=args.mix_switch_prob)
    optimizer = _make_optimizer(args, model.parameters(),
                                compute_dtype if compute_dtype != torch.float32 else None)
    scheduled = not isinstance(optimizer, SGD) and (
        args.lr_schedule != "constant" or args.lr_warmup_steps > 0)
    ema = None
    if args.model_ema_decay > 0:
        from mipipe.optim import ModelEMA
        ema = ModelEMA(model, decay=args.model_ema_decay, every=args.model_ema_steps,
                       warmup=bool(args.model_ema_warmup))

    start_epoch = 0
    if args.resume:
        path = ckpt.resolve_resume_path(args.resume, args.model_dir)
        if path and os.path.isfile(path):
            print(f"=> loading checkpoint '{path}'")
            state = ckpt.load_checkpoint(path, device)
            start_epoch = int(state["epoch"])
            best_acc1 = float(state.get("best_acc1", 0.0))
            ckpt.load_model_state(model, state["state_dict"])
            ckpt.restore_model_step(model, state)
            optimizer.load_state_dict(state["optimizer"])
            if ema is not None:
                if "model_ema" in state:
                    asked = (ema.decay, ema.every, ema.warmup)
                    ema.load_state_dict(state["model_ema"])
                    # the average goes on as it was being taken: the checkpoint's settings win
                    if asked != (ema.decay, ema.every, ema.warmup):
                        print(f"=> model EMA: the checkpoint's decay / steps / warmup "
                              f"{(ema.decay, ema.every, ema.warmup)} replace the command line's "
                              f"{asked}", flush=True)
                else:  # a run that had no EMA: the average starts from the loaded weights
                    ema.reset()
            print(f"=> loaded checkpoint '{path}' (epoch {start_epoch})")
        else:
            print(f"=> no checkpoint found at '{path}'")

    train_files = test_files = []
    if args.data_dir:
        from mipipe.data import records as REC
        train_files = REC.dataset_files(args.data_dir, args.dataset, "train")
        test_files = REC.dataset_files(args.data_dir, args.dataset, "test")
        if not train_files:
            raise FileNotFoundError(f"no {args.dataset} record files in {args.data_dir}")
    if train_files:
        # task.py:246-267: RandomCrop(32, 4) + flip + Normalize, DistributedSampler shards,
        # test loader batch 128 unshuffled — on the native multi-threaded loader
        from mipipe.data import records as REC
        mean, std = {"mnist": (REC.MNIST_MEAN, REC.MNIST_STD),
                     "imagenet": (REC.IMAGENET_MEAN, REC.IMAGENET_STD)}.get(
                         args.dataset, (REC.CIFAR10_MEAN, REC.CIFAR10_STD))
        if manifest is not None and "mean" in manifest and "std" in manifest:
            mean, std = tuple(manifest["mean"]), tuple(manifest["std"])
        pad = 4 if args.dataset == "cifar10" else 0
        decode = "device" if args.device_decode else "host"
        # rrc: RandomResizedCrop + flip (train) / 7/8 centre crop (test) to the model's size
        rkw = {"label_bytes": label_bytes}
        if record_transform == "rrc":
            rkw.update(transform="rrc", out_size=(H, W))
        akw = {}
        if augmenting:
            akw = {"auto_augment": None if args.auto_augment == "none" else args.auto_augment,
                   "random_erase": args.random_erase}
            print(f"=> record augmentation: auto_augment={args.auto_augment} "
                  f"random_erase={args.random_erase} (augment -> {record_transform} -> erase, "
                  f"decode={decode})", flush=True)
        probe = REC.RecordDataLoader(train_files, stored, args.batch_size, train=True,
                                     pad=pad, mean=mean, std=std, seed=args.random_seed,
                                     workers=max(1, args.workers), device=device, decode=decode,
                                     **rkw, **akw)
        train_sampler = DistributedSampler(probe.num_samples_total, seed=args.random_seed)
        probe.sampler = train_sampler
        train_loader = probe
        tfiles = test_files or train_files
        test_loader = REC.RecordDataLoader(tfiles, stored, 128, train=False, mean=mean,
                                           std=std, workers=max(1, args.workers), device=device,
                                           decode=decode, **rkw)
        test_sampler = DistributedSampler(test_loader.num_samples_total, shuffle=False)
        test_loader.sampler = test_sampler
    else:
        train_n = args.train_samples or N
        test_n = args.test_samples or min(N, 10000)
        train_set = SyntheticImageDataset(args.dataset, train_n, seed=args.random_seed,
                                          shape=(C, H, W), num_classes=K)
        test_set = SyntheticImageDataset(args.dataset, test_n, seed=args.random_seed,
                                         shape=(C, H, W), num_classes=K)
        train_sampler = DistributedSampler(train_set, seed=args.random_seed)
        test_sampler = DistributedSampler(test_set, shuffle=False)
        train_loader = DeviceBatchLoader(train_set, args.batch_size, train_sampler, device)
        test_loader = DeviceBatchLoader(test_set, 128, test_sampler, device)

    if not isinstance(optimizer, (SGD, AdamW)) and args.lr_total_steps is None \
            and start_epoch == 0:
        # the schedule ends with the run (its parameters are read from the group at every step)
        per_epoch = min(len(train_loader), args.steps) if args.steps else len(train_loader)
        optimizer.param_groups[0]["total_steps"] = args.num_epochs * per_epoch
    meter = ThroughputMeter(device, warmup_steps=args.warmup_steps)
    jlog = JsonlLogger(args.rank, args.log_dir or None)
    if args.trace:
        trace.enable(True)
    global_step = 0
    last_loss = float("nan")
    accuracy = None
    # --hip-graph: the first full-size batch runs eagerly inside GraphedStep (a real training
    # step: warmup=1), which then captures the step; later batches of that shape replay it
    graphed, graph_shape = None, None
    if args.hip_graph:
        from mipipe.train.graph import GraphedStep, graph_safe
        ok, why = graph_safe(_unwrap(model), optimizer) if use_gpu else (False, "no GPU")
        if isinstance(model, DataParallel):
            ok, why = False, "DataParallel runs replicas on host threads"
        if not ok:
            print(f"=> --hip-graph off: {why}", flush=True)
            args.hip_graph = False

    def _train_step(x, y, mix=None):
        optimizer.zero_grad()
        if mix is not None:
            MK.batch_mix(x, mix, out=x)  # x is the captured step's own static buffer
        loss_ = criterion(model(x), y, mix)
        loss_.backward()
        optimizer.step()
        if ema is not None:
            ema.update()
        return loss_

    fused = bool(args.fused_eval) or inference.is_fused_eval()

    eval_meter = None
    if args.eval_metrics == "full":
        from mipipe.metrics import CONFUSION_MAX_CLASSES, EvalMeter
        ncls = kw.get("num_classes", 1000)  # every model but mnist_cnn defaults to 1000 classes
        eval_meter = EvalMeter(ncls, topk=args.eval_topk, confusion=ncls <= CONFUSION_MAX_CLASSES,
                               device=device)
    eval_full = {}  # the last evaluation's EvalMeter results: "" live model, "_ema" averaged

    def _evaluate():
        """(accuracy of the live model, accuracy of the averaged one or None)."""
        with inference.fused_eval(fused):
            if eval_meter is not None:
                eval_full[""] = evaluate_full(model, device, test_loader, eval_meter)
                if ema is None:
                    return eval_full[""]["accuracy"], None
                with ema.swapped():
                    eval_full["_ema"] = evaluate_full(model, device, test_loader, eval_meter)
                return eval_full[""]["accuracy"], eval_full["_ema"]["accuracy"]
            acc = evaluate(model, device, test_loader)
            if ema is None:
                return acc, None
            with ema.swapped():
                return acc, evaluate(model, device, test_loader)

    def _full_txt():
        if eval_meter is None:
            return ""
        k, res = eval_meter.topk, eval_full[""]
        return f", Top-{k}: {res[f'accuracy_top{k}']}, Loss: {res['loss']:.4f}"

    def _ema_txt(acc_ema):
        return "" if ema is None else f", Accuracy EMA: {acc_ema} ({ema.num_updates()} updates)"

    for epoch in range(start_epoch, args.num_epochs):
        epoch_start = datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
        print(f"Rank: {args.rank}, Epoch: {epoch}, Training start: {epoch_start}", flush=True)
        train_sampler.set_epoch(epoch)
        if epoch % args.eval_every == 0:
            accuracy, accuracy_ema = _evaluate()
            if args.rank == 0:
                ckpt.export_model(model, args, epoch, accuracy, ema, accuracy_ema)
                print("-" * 75)
                print(f"Epoch: {epoch}, Accuracy: {accuracy}{_full_txt()}{_ema_txt(accuracy_ema)}, Time: "
                      f"{datetime.now().strftime('%Y_%m_%d_%H_%M_%S')}")
                print("-" * 75, flush=True)
        model.train()
        it = iter(train_loader)
        i = 0
        while True:
            if args.steps and i >= args.steps:
                break
            with trace.phase("data"):
                batch = next(it, None)
            if batch is None:
                break
            inputs, labels = batch
            _fault_check(args.rank, global_step)
            meter.step_begin()
            extra = ()
            if mixer is not None:  # one 32-byte upload; the kernels read it on the device
                extra = (mixer.descriptor(epoch, i, inputs.shape[-2], inputs.shape[-1]),)
            if args.hip_graph and (graphed is None or tuple(inputs.shape) == graph_shape):
                with trace.phase("graph_step"):
                    if graphed is None:
                        graphed = GraphedStep(_train_step, (inputs, labels) + extra, warmup=1)
                        graph_shape = tuple(inputs.shape)
                        loss = graphed.warmup_loss  # the eager warm-up step trained this batch
                    else:
                        loss = graphed.step(inputs, labels, *extra)
            else:
                with trace.phase("zero_grad"):
                    optimizer.zero_grad()
                with trace.phase("forward"):
                    if mixer is not None:
                        # out of place: the loader may yield this batch again (cached batches)
                        inputs = MK.batch_mix(inputs.contiguous(), extra[0])
                    outputs = model(inputs)
                    loss = criterion(outputs, labels, *extra)
                with trace.phase("backward+allreduce"):
                    loss.backward()
                with trace.phase("optimizer"):
                    optimizer.step()
                    if ema is not None:
                        ema.update()
            meter.step_end(inputs.shape[0])
            global_step += 1
            i += 1
            if args.log_every and global_step % args.log_every == 0:
                if isinstance(model, DistributedDataParallel):
                    model.check_comm_errors()  # a one-shot wait that gave up -> error, no sync
                last_loss = float(loss.detach().float().item())
                # the LR the last step used, as its kernels computed it on the device
                lr_kw = {"lr": float(optimizer.last_lr().item())} if scheduled else {}
                if mixer is not None:
                    lr_kw.update(mix_mode=mixer.last_mode, mix_lambda=mixer.last_lambda)
                jlog.log("step", epoch=epoch, step=global_step, loss=last_loss,
                         samples_per_sec=meter.samples_per_sec(), **lr_kw)
                if args.rank == 0:
                    lr_txt = f" lr {lr_kw['lr']:.6g}" if scheduled else ""
                    if mixer is not None:
                        lr_txt += f" mix {mixer.last_mode} lambda {mixer.last_lambda:.4f}"
                    print(f"epoch {epoch} step {global_step} loss {last_loss:.4f}{lr_txt} "
                          f"{meter.samples_per_sec() * world:.1f} samples/s (job)", flush=True)
        if args.rank == 0:
            ckpt.save_checkpoint(model, optimizer, args, epoch + 1, best_acc1, ema)
    if isinstance(model, DistributedDataParallel):
        model.check_comm_errors(final=True)
    # fixed quirk: evaluate and save the *trained* model at the end as well
    accuracy, accuracy_ema = _evaluate()
    best_acc1 = max(best_acc1, accuracy)
    last_loss = float(loss.detach().float().item()) if global_step else last_loss
    metrics = {"accuracy": accuracy, "loss": last_loss, "epochs": args.num_epochs,
               "steps": global_step, "world_size": world, "arch": args.arch,
               "batch_per_process": args.batch_size, "global_batch": args.batch_size * world,
               "samples_per_sec_per_rank": meter.samples_per_sec(),
               "samples_per_sec_job": meter.samples_per_sec() * world,
               "dtype": str(compute_dtype).replace("torch.", ""), "device": str(device),
               "backend": (torch.distributed.get_backend() if args.distributed else "none"),
               "hip_graph": bool(args.hip_graph), "deterministic": bool(args.deterministic),
               "fused_eval": fused}
    if stochastic_depth is not None:
        metrics["stochastic_depth"] = stochastic_depth
    if scheduled:
        metrics["lr"] = float(optimizer.last_lr().item())
    if mixer is not None:
        metrics.update(mix_mode=mixer.last_mode, mix_lambda=mixer.last_lambda)
    if augmenting:
        metrics.update(auto_augment=args.auto_augment, random_erase=args.random_erase)
    if ema is not None:
        metrics.update(accuracy_ema=accuracy_ema, ema_updates=ema.num_updates())
    if eval_meter is not None:
        for suffix, res in eval_full.items():
            metrics.update(_full_metrics(res, eval_meter.topk, suffix))
        if args.rank == 0 and args.eval_report:
            ckpt.write_json(args.eval_report, eval_full[""] if ema is None else
                            {**eval_full[""], "ema": eval_full["_ema"]})
    if args.rank == 0:
        ckpt.export_model(model, args, args.num_epochs, accuracy, ema, accuracy_ema)
        ckpt.save_checkpoint(model, optimizer, args, args.num_epochs, best_acc1, ema)
        print("MIPIPE_METRICS " + json.dumps(metrics), flush=True)
        if args.metrics_file:
            ckpt.write_json(args.metrics_file, metrics)
    jlog.log("final", **metrics)
    jlog.close()
    epoch_end = datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
    print(f"Epoch complete: {epoch_end}", flush=True)
    dist_utils.barrier(device if use_gpu else None)
    dist_utils.cleanup()
    return metrics


if __name__ == "__main__":
    sys.exit(main())
