"""eval_stats on the CPU: the reference contract (mipipe.ops._ref.eval_stats) against torch in
float64 and against hand-written expectations for the tie / NaN / invalid-label rules,
mipipe.metrics.EvalMeter's derived metrics, its all-reduce over two gloo ranks, and the
``--eval-metrics full`` path of task.py and of the three-step pipeline."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from eval_stats_common import IGNORE, make_inputs, special_rows
from mipipe.metrics import EvalMeter, derive_metrics
from mipipe.ops import _ref
from mipipe.ops import kernels as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))

TOL = 1e-4  # the project's fp32-vs-float64 tolerance (tests/test_fp32_gpu.py)
Q24 = float(1 << 24)


def _buffers(Vv, bins=15):
    return (torch.zeros(8, dtype=torch.int64), torch.zeros(Vv, Vv, dtype=torch.int32),
            torch.zeros(3, bins, dtype=torch.int64))


@pytest.mark.parametrize("V", [10, 1000])
def test_ref_against_float64(V):
    R = 257
    g = torch.Generator().manual_seed(V)
    # a random permutation of V distinct values per row (fp32 randn rows of 1000 do tie)
    x = torch.stack([torch.randperm(V, generator=g) for _ in range(R)]).float() * (12.0 / V) - 6
    assert all(len(torch.unique(r)) == V for r in x), "the random logits must be tie-free"
    y = torch.randint(0, V, (R,), generator=g)
    y[::4] = x[::4].argmax(1)
    xd = x.double()
    pred = xd.argmax(1)
    for k in (1, 5, V):
        c, cm, h = _buffers(V)
        K.eval_stats(x, y, c, cm, h, k=k)  # CPU tensors: dispatches to _ref.eval_stats
        topk = (xd.topk(k, 1).indices == y[:, None]).any(1).sum().item()
        assert c.tolist()[:5] == [R, (pred == y).sum().item(), topk, 0, 0]
        assert torch.equal(cm.long().reshape(-1), torch.bincount(y * V + pred, minlength=V * V))
        loss = F.cross_entropy(xd, y, reduction="sum").item()
        assert abs(c[5].item() / Q24 - loss) / loss < TOL
        assert h[:2].sum().item() == R and h[1].sum().item() == c[1].item()
        conf = torch.softmax(xd, 1).max(1).values.sum().item()
        assert abs(h[2].sum().item() / Q24 - conf) / conf < TOL
    with pytest.raises(ValueError):
        _ref.eval_stats(x, y, c, k=V + 1)
    with pytest.raises(ValueError):
        _ref.eval_stats(x, y, c, k=0)


@pytest.mark.parametrize("V,valid_cols", [(10, -1), (16, 10), (1003, -1)])
@pytest.mark.parametrize("k", [1, 5])
def test_ref_rules_row_by_row(V, valid_cols, k):
    Vv = valid_cols if valid_cols > 0 else V
    for x, y, want in special_rows(V, Vv):
        c, cm, h = _buffers(Vv)
        _ref.eval_stats(x[None], torch.tensor([y]), c, cm, h, k=k, ignore_index=IGNORE,
                        valid_cols=valid_cols)
        what = (x[:8].tolist(), y)
        if want == "skip":
            assert c.tolist() == [0] * 8 and not cm.any() and not h.any(), what
        elif want == "invalid":
            assert c.tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and not cm.any() and not h.any(), what
        else:
            pred, rank, finite = want
            assert c.tolist()[:5] == [1, int(rank == 0), int(rank < k), int(not finite), 0], what
            assert cm.sum().item() == 1 and cm[y, pred].item() == 1, what
            assert (pred == y) == (rank == 0), what
            assert h[:2].sum().item() == int(finite) and h[1].sum().item() == int(finite and rank == 0)
            if finite:
                xd = x[:Vv].double()
                loss = (torch.logsumexp(xd, 0) - xd[y]).item()
                assert abs(c[5].item() / Q24 - loss) <= TOL * max(loss, 1e-3), what
            else:
                assert c[5].item() == 0 and h[2].sum().item() == 0, what
    # all special rows in one call: the sums of the single rows
    xs = torch.stack([r[0] for r in special_rows(V, Vv)])
    ys = torch.tensor([r[1] for r in special_rows(V, Vv)])
    c, cm, h = _buffers(Vv)
    _ref.eval_stats(xs, ys, c, cm, h, k=k, valid_cols=valid_cols)
    wants = [r[2] for r in special_rows(V, Vv)]
    rows = [w for w in wants if isinstance(w, tuple)]
    assert c.tolist()[:5] == [len(rows), sum(w[1] == 0 for w in rows), sum(w[1] < k for w in rows),
                              sum(not w[2] for w in rows), wants.count("invalid")]
    assert cm.sum().item() == len(rows) and h[:2].sum().item() == sum(w[2] for w in rows)


def test_derived_metrics_from_confusion():
    # labels in rows, predictions in columns; class 2 has no samples and no predictions
    cm = [[3, 1, 0],
          [2, 4, 0],
          [0, 0, 0]]
    counters = [10, 7, 10, 0, 0, int(round(12.5 * Q24)), 0, 0]
    res = derive_metrics(counters, None, cm, topk=2)
    assert res["rows"] == 10 and res["accuracy"] == 0.7 and res["accuracy_top2"] == 1.0
    assert res["loss"] == 1.25 and res["nonfinite"] == 0 and res["invalid"] == 0
    assert res["confusion"] == cm and res["support"] == [4, 6, 0]
    assert res["recall"] == pytest.approx([3 / 4, 4 / 6, 0.0])
    assert res["precision"] == pytest.approx([3 / 5, 4 / 5, 0.0])
    f1 = [2 * 3 / (4 + 5), 2 * 4 / (6 + 5)]
    assert res["f1"] == pytest.approx(f1 + [0.0])
    assert res["balanced_accuracy"] == pytest.approx((3 / 4 + 4 / 6) / 2)  # class 2 left out
    assert res["macro_f1"] == pytest.approx(sum(f1) / 2)
    assert "ece" not in res and "confidence_curve" not in res


@pytest.mark.parametrize("bins", [15, 64])
def test_ece_and_curve_against_numpy(bins):
    logits, labels = make_inputs(torch.float32, 777, 10, -1)
    meter = EvalMeter(10, topk=3, bins=bins)
    meter.update(logits[:400], labels[:400])
    meter.update(logits[400:], labels[400:])
    res = meter.result()
    # raw fp32 confidences of the rows the histogram holds (finite loss, valid label)
    ok = (labels >= 0) & (labels < 10)
    x, y = logits[ok], labels[ok]
    lse = torch.logsumexp(x, 1)
    fin = torch.isfinite(lse - x.gather(1, y[:, None])[:, 0])
    conf = torch.exp(x[fin].max(1).values - lse[fin]).numpy()
    hit = (x[fin].argmax(1) == y[fin]).numpy()
    b = np.minimum(bins - 1, np.floor(conf * np.float32(bins)).astype(np.int64))
    n = len(conf)
    ece = sum(abs(hit[b == i].mean() - conf[b == i].astype(np.float64).mean()) * (b == i).sum() / n
              for i in range(bins) if (b == i).any())
    assert res["ece"] == pytest.approx(ece, rel=1e-5, abs=1e-7)
    assert len(res["confidence_curve"]) == bins
    for i, (thr, share, acc) in enumerate(res["confidence_curve"]):
        sel = b >= i
        assert thr == i / bins and share == pytest.approx(sel.sum() / n)
        assert acc == pytest.approx(hit[sel].mean() if sel.any() else 0.0)
    assert res["confidence_curve"][0][1] == 1.0
    assert res["rows"] == int(ok.sum()) and res["nonfinite"] == int((~fin).sum())
    assert res["invalid"] == 4 and res["accuracy_top3"] >= res["accuracy"]


def test_log_to_fills_classification_metrics():
    from mipipe.dsl.types import ClassificationMetrics
    logits, labels = make_inputs(torch.float32, 777, 10, -1)
    meter = EvalMeter(10, bins=15)
    meter.update(logits, labels)
    art = ClassificationMetrics(name="m", uri="")
    res = meter.log_to(art)
    cm = art.metadata["confusionMatrix"]
    assert [s["displayName"] for s in cm["annotationSpecs"]] == [str(i) for i in range(10)]
    assert [r["row"] for r in cm["rows"]] == res["confusion"]
    assert sum(sum(r["row"]) for r in cm["rows"]) == res["rows"]
    pts = art.metadata["confidenceMetrics"]
    assert len(pts) == 15
    for p, (thr, share, acc) in zip(pts, res["confidence_curve"]):
        assert p == {"confidenceThreshold": thr, "recall": share, "falsePositiveRate": 1.0 - acc}
    # reset zeroes in place
    ptrs = (meter.counters.data_ptr(), meter.hist.data_ptr(), meter.confusion.data_ptr())
    meter.reset()
    assert ptrs == (meter.counters.data_ptr(), meter.hist.data_ptr(), meter.confusion.data_ptr())
    assert not meter.counters.any() and not meter.hist.any() and not meter.confusion.any()
    # no confusion matrix: only the curve is logged; topk is clamped to the class count
    small = EvalMeter(10, topk=50, confusion=False)
    assert small.topk == 10
    small.update(logits, labels)
    art2 = ClassificationMetrics(name="m2", uri="")
    small.log_to(art2)
    assert "confusionMatrix" not in art2.metadata and len(art2.metadata["confidenceMetrics"]) == 15


def _meter_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    logits, labels = make_inputs(torch.float32, 777, 10, -1)
    meter = EvalMeter(10, topk=3)
    half = 389
    sl = slice(0, half) if rank == 0 else slice(half, None)
    meter.update(logits[sl], labels[sl])
    meter.all_reduce()
    out[rank] = (meter.counters.clone(), meter.hist.clone(), meter.confusion.clone(),
                 meter.result())
    dist.destroy_process_group()


def test_all_reduce_two_ranks_gloo():
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_meter_worker, args=(world, 29500 + os.getpid() % 400, out), nprocs=world, join=True)
    logits, labels = make_inputs(torch.float32, 777, 10, -1)
    one = EvalMeter(10, topk=3)
    one.update(logits, labels)
    one.all_reduce()  # no process group: a no-op
    want = one.result()
    for r in range(world):
        c, h, cm, res = out[r]
        assert torch.equal(c, one.counters), (r, c, one.counters)  # the Q24 loss bit for bit
        assert torch.equal(h, one.hist) and torch.equal(cm, one.confusion)
        assert cm.dtype == torch.int32
        assert res == want


TODAYS_KEYS = {"accuracy", "loss", "epochs", "steps", "world_size", "arch", "batch_per_process",
               "global_batch", "samples_per_sec_per_rank", "samples_per_sec_job", "dtype",
               "device", "backend", "hip_graph", "deterministic", "fused_eval"}
FULL_KEYS = {"accuracy_top5", "eval_loss", "ece", "macro_f1", "balanced_accuracy"}


def test_task_eval_metrics_full_cpu(tmp_path, monkeypatch, capsys):
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    def run(tag, *extra):
        mfile = tmp_path / f"{tag}.json"
        args = ["--arch", "mnist_cnn", "--dataset", "mnist", "--batch_size", "32",
                "--train-samples", "128", "--test-samples", "64", "--local_training",
                "--model_dir", str(tmp_path / tag), "--learning_rate", "0.05", "--log-every", "0",
                "--num_epochs", "1", "--metrics-file", str(mfile)]
        assert T.main(args + list(extra)) == 0
        return json.loads(mfile.read_text())

    top1 = run("top1")
    assert set(top1) == TODAYS_KEYS
    assert not (tmp_path / "report.json").exists()
    capsys.readouterr()
    full = run("full", "--eval-metrics", "full", "--eval-report", str(tmp_path / "report.json"))
    assert set(full) == TODAYS_KEYS | FULL_KEYS
    assert full["accuracy"] == top1["accuracy"]
    assert 0.0 <= full["accuracy"] <= full["accuracy_top5"] <= 1.0
    assert full["eval_loss"] > 0 and 0.0 <= full["ece"] <= 1.0
    assert "Top-5: " in capsys.readouterr().out
    rep = json.loads((tmp_path / "report.json").read_text())
    assert sum(sum(r) for r in rep["confusion"]) == 64 == rep["rows"]
    assert rep["accuracy"] == full["accuracy"] and rep["loss"] == full["eval_loss"]
    assert len(rep["confidence_curve"]) == 15 and len(rep["recall"]) == 10
    # with a weight EMA: the same keys once more, suffixed _ema
    ema = run("ema", "--eval-metrics", "full", "--eval-topk", "3", "--model-ema-decay", "0.9")
    k3 = {k.replace("top5", "top3") for k in FULL_KEYS}
    assert set(ema) == TODAYS_KEYS | k3 | {k + "_ema" for k in k3} | {"accuracy_ema", "ema_updates"}
    assert ema["accuracy"] == top1["accuracy"]


def test_three_step_pipeline_logs_full_metrics(tmp_path, gcs_root):
    import three_step_pipeline as P
    rc = P.main(["--gpus", "0", "--arch", "mnist_cnn", "--dataset", "mnist", "--epochs", "1",
                 "--batch-size", "64", "--n-train", "128", "--n-test", "96", "--lr", "0.05",
                 "--baseline-accuracy", "101", "--serving-dir", str(tmp_path / "serving"),
                 "--spec", str(tmp_path / "spec.json")])
    assert rc == 0
    runs = [os.path.join(r, "run.json") for r, _, fs in os.walk(gcs_root) if "run.json" in fs]
    assert len(runs) == 1
    outputs = json.load(open(runs[0]))["tasks"]["evaluate"]["outputs"]
    meta = outputs["artifacts"]["metrics"][0]["metadata"]
    rows = [r["row"] for r in meta["confusionMatrix"]["rows"]]
    assert sum(sum(r) for r in rows) == 96
    assert len(meta["confidenceMetrics"]) == 15
    assert {"confidenceThreshold", "recall", "falsePositiveRate"} == set(meta["confidenceMetrics"][0])
    summ = outputs["artifacts"]["summary"][0]["metadata"]
    assert {"accuracy", "baseline_accuracy", "deploy", "loss", "accuracy_top5", "ece"} <= set(summ)
    hits = sum(r[i] for i, r in enumerate(rows))
    assert summ["accuracy"] == 100.0 * hits / 96
