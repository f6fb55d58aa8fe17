"""The eval_stats kernel (csrc/kernels/eval_stats.hip) and mipipe.metrics.EvalMeter on the MI355X:
integer results bit for bit against the reference contract, loss and confidence sums against
float64, null buffers, atomic contention, agreement with top1_correct, reproducibility over batch
splits, evaluation of a weight EMA and ``task.py --eval-metrics full``.
Run on an MI355X:  python -m pytest tests -m gpu
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from eval_stats_common import IGNORE, f64_stats, make_inputs, near_bin_edge
from mipipe.metrics import EvalMeter
from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4  # the project's fp32-vs-float64 tolerance (tests/test_fp32_gpu.py)
Q24 = float(1 << 24)
SHAPES = [(1, 10, -1), (5, 10, -1), (777, 10, -1), (777, 1000, -1), (777, 1003, -1),
          (33, 30528, 30522)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    yield


def _buffers(Vv, bins, dev="cuda", cm=True, hist=True):
    return (torch.zeros(8, dtype=torch.int64, device=dev),
            torch.zeros(Vv, Vv, dtype=torch.int32, device=dev) if cm else None,
            torch.zeros(3, bins, dtype=torch.int64, device=dev) if hist else None)


def _snapshot(*bufs):
    return [None if b is None else b.cpu().clone() for b in bufs]


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("R,V,valid_cols", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_bits_against_reference(dtype, R, V, valid_cols, k):
    """Two launches into the same buffers.  Counters, histogram counts and the confusion matrix
    equal the reference exactly; the Q24 loss and confidence sums are within 1e-4 of float64.
    Rows whose float64 conf * bins lies within 1e-3 of an integer (for either bin count) are taken
    out on the CPU, by relabelling them ignore_index so that R and the block layout stay; fp32 and
    float64 confidences differ by at most 4.3e-5 bin units."""
    Vv = valid_cols if valid_cols > 0 else V
    logits, labels = make_inputs(dtype, R, V, valid_cols)
    st = f64_stats(logits, labels, valid_cols, 15)
    near = near_bin_edge(st["conf"], 15) | near_bin_edge(st["conf"], 64)
    print(f"dropped {int(near.sum())} of {R} rows")
    assert int(near.sum()) <= 0.02 * R
    labels = torch.where(near, torch.full_like(labels, IGNORE), labels)
    fin = st["finite"] & ~near
    with_cm = Vv <= 4096  # V = 30528: the confusion pointer is null
    dl, dy = logits.cuda(), labels.cuda()
    for bins in (15, 64):
        rc, rcm, rh = _buffers(Vv, bins, "cpu", cm=with_cm)
        _ref.eval_stats(logits, labels, rc, rcm, rh, k, IGNORE, valid_cols)
        c, cm, h = _buffers(Vv, bins, cm=with_cm)
        for _ in range(2):
            K.eval_stats(dl, dy, c, cm, h, k=k, ignore_index=IGNORE, valid_cols=valid_cols)
        c, cm, h = _snapshot(c, cm, h)
        assert c[:5].tolist() == (2 * rc[:5]).tolist() and c[6:].tolist() == [0, 0]
        assert torch.equal(h[:2], 2 * rh[:2])
        if with_cm:
            assert torch.equal(cm, 2 * rcm)
        loss64 = 2 * st["loss"][fin].sum().item()
        print(f"bins {bins}: loss {c[5].item() / Q24} float64 {loss64}")
        assert abs(c[5].item() / Q24 - loss64) <= TOL * loss64
        b64 = torch.floor(st["conf"][fin] * bins).clamp(0, bins - 1).long()
        conf64 = 2 * torch.zeros(bins, dtype=torch.float64).index_add_(0, b64, st["conf"][fin])
        assert torch.equal(torch.bincount(b64, minlength=bins) * 2, h[0] + h[1])
        got = h[2].double() / Q24
        assert bool(((got - conf64).abs() <= TOL * conf64).all()), (got, conf64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_null_buffers(dtype):
    logits, labels = make_inputs(dtype, 777, 1000, -1)
    dl, dy = logits.cuda(), labels.cuda()
    got = []
    for cm_on, hist_on in ((True, True), (True, False), (False, True), (False, False)):
        c, cm, h = _buffers(1000, 15, cm=cm_on, hist=hist_on)
        K.eval_stats(dl, dy, c, cm, h, k=5)
        got.append(_snapshot(c, cm, h))
    for c, cm, h in got[1:]:
        assert torch.equal(c, got[0][0])
        assert cm is None or torch.equal(cm, got[0][1])
        assert h is None or torch.equal(h, got[0][2])
    assert got[0][0][0].item() > 700 and got[0][1].sum().item() == got[0][0][0].item()


def test_contention_one_cell():
    R, V = 1024, 1000
    row = torch.randn(V, generator=torch.Generator().manual_seed(5)) * 3
    pred = int(row.argmax())
    logits = row.repeat(R, 1).cuda()
    labels = torch.full((R,), 7, dtype=torch.int64, device="cuda")
    c, cm, h = _buffers(V, 15)
    K.eval_stats(logits, labels, c, cm, h, k=5)
    c, cm, h = _snapshot(c, cm, h)
    assert pred != 7 and cm[7, pred].item() == R and cm.sum().item() == R
    assert c[:5].tolist() == [R, 0, c[2].item(), 0, 0] and c[2].item() in (0, R)
    assert h[0].max().item() == R and h[0].sum().item() == R and h[1].sum().item() == 0
    conf = torch.softmax(row.double(), 0).max().item()
    b = int(h[0].argmax())
    assert b == min(14, int(conf * 15)) and abs(h[2, b].item() / Q24 / R - conf) < TOL * conf
    assert h[2].sum().item() == h[2, b].item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [10, 1000])
def test_agrees_with_top1_correct(dtype, V):
    """The inputs of tests/test_fp32_gpu.py::test_top1_correct, with NaN rows added."""
    torch.manual_seed(4321)
    R = 777
    logits = torch.randn(R, V, device="cuda").to(dtype)
    logits[::7, 3] = logits[::7].float().max(1).values.to(dtype)  # ties: first index wins
    labels = torch.randint(0, V, (R,), device="cuda")
    labels[::5] = logits[::5].float().argmax(1)
    logits[::11, 5] = float("nan")  # NaN counts as maximal
    logits[::33, 2] = float("nan")  # two NaNs: the first one is the prediction
    labels[::22] = 5
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    native().top1_correct(logits, labels, out)
    c, _, _ = _buffers(V, 15, cm=False, hist=False)
    K.eval_stats(logits, labels, c, k=1)
    assert c[1].item() == out.item() > 0
    assert c[0].item() == R and c[2].item() == c[1].item()


@pytest.mark.parametrize("R,V,valid_cols", [(777, 10, -1), (777, 1003, -1), (33, 30528, 30522)])
def test_topk_limits(R, V, valid_cols):
    Vv = valid_cols if valid_cols > 0 else V
    logits, labels = make_inputs(torch.bfloat16, R, V, valid_cols)
    dl, dy = logits.cuda(), labels.cuda()
    c, _, _ = _buffers(Vv, 15, cm=False, hist=False)
    K.eval_stats(dl, dy, c, k=Vv, valid_cols=valid_cols)
    assert c[2].item() == c[0].item() > 0
    c1, _, _ = _buffers(Vv, 15, cm=False, hist=False)
    K.eval_stats(dl, dy, c1, k=1, valid_cols=valid_cols)
    assert c1[2].item() == c1[1].item() and c1[0].item() == c[0].item()
    with pytest.raises(RuntimeError):
        K.eval_stats(dl, dy, c, k=Vv + 1, valid_cols=valid_cols)
    with pytest.raises(RuntimeError):
        K.eval_stats(dl, dy, c, k=0, valid_cols=valid_cols)


def test_reproducible_over_runs_and_batch_splits():
    logits, labels = make_inputs(torch.bfloat16, 777, 1000, -1)
    dl, dy = logits.cuda(), labels.cuda()
    results = []
    for nb in (1, 1, 3, 7):
        c, cm, h = _buffers(1000, 15)
        for xs, ys in zip(dl.chunk(nb), dy.chunk(nb)):
            K.eval_stats(xs, ys, c, cm, h, k=5)
        results.append(_snapshot(c, cm, h))
    for got in results[1:]:
        for a, b in zip(got, results[0]):
            assert torch.equal(a, b)
    # an empty batch launches nothing
    c, cm, h = _buffers(1000, 15)
    K.eval_stats(dl[:0], dy[:0], c, cm, h, k=5)
    assert not c.any() and not cm.any() and not h.any()


def _aten_stats(model, x, y, k):
    with torch.no_grad():
        L = torch.cat([model(xs).float() for xs in x.chunk(2)])
    ly = L.gather(1, y[:, None])
    cols = torch.arange(L.shape[1], device=L.device)
    rank = (L > ly).sum(1) + ((L == ly) & (cols[None] < y[:, None])).sum(1)
    pred = L.argmax(1)
    return {"logits": L, "top1": int((pred == y).sum()), "topk": int((rank < k).sum()),
            "cm": torch.bincount(y * L.shape[1] + pred, minlength=L.shape[1] ** 2).cpu(),
            "loss": F.cross_entropy(L.double(), y).item()}


def _check_meter(meter, model, x, y, want):
    meter.reset()
    with torch.no_grad():
        for xs, ys in zip(x.chunk(2), y.chunk(2)):
            meter.update(model(xs), ys)
    res = meter.result()
    n = y.numel()
    assert res["rows"] == n and res["nonfinite"] == 0 and res["invalid"] == 0
    assert res["accuracy"] == want["top1"] / n and res["accuracy_top3"] == want["topk"] / n
    assert torch.equal(torch.tensor(res["confusion"]).reshape(-1), want["cm"])
    assert abs(res["loss"] - want["loss"]) <= TOL * want["loss"]
    assert 0.0 <= res["ece"] <= 1.0 and len(res["confidence_curve"]) == 15


def test_eval_meter_resnet18_and_ema():
    from mipipe.models import create_model
    from mipipe.ops.determinism import deterministic
    from mipipe.ops.functional import cross_entropy
    from mipipe.optim import SGD, ModelEMA
    with deterministic(True):
        torch.manual_seed(0)
        model = create_model("resnet18", num_classes=10).cuda()
        opt = SGD(model.parameters(), lr=0.05, momentum=0.9)
        ema = ModelEMA(model, decay=0.5, every=1, warmup=False)
        x = torch.randn(64, 3, 32, 32, device="cuda")
        y = torch.randint(0, 10, (64,), device="cuda")
        for _ in range(3):
            opt.zero_grad()
            cross_entropy(model(x[:16]), y[:16]).backward()
            opt.step()
            ema.update()
        model.eval()
        meter = EvalMeter(10, topk=3, device="cuda")
        live = _aten_stats(model, x, y, 3)
        _check_meter(meter, model, x, y, live)
        with ema.swapped():
            avg = _aten_stats(model, x, y, 3)
            _check_meter(meter, model, x, y, avg)
        assert not torch.equal(avg["logits"], live["logits"])
        _check_meter(meter, model, x, y, live)


def _task(tmp_path, tag, *extra):
    from mipipe.launch.launcher import free_port
    env = dict(os.environ)
    for key in ("LOCAL_RANK", "GROUP_RANK"):
        env.pop(key, None)
    env.update({"WORLD_SIZE": "1", "RANK": "0", "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": str(free_port()), "HSA_ENABLE_IPC_MODE_LEGACY": "0",
                "PYTHONPATH": REPO + os.pathsep + env.get("PYTHONPATH", "")})
    mfile = tmp_path / f"{tag}.json"
    args = ["--num_epochs=1", "--local_training", "--model_dir", str(tmp_path / tag),
            "--batch_size", "256", "--train-samples", "1024", "--test-samples", "256",
            "--hip-graph", "--metrics-file", str(mfile)] + list(extra)
    r = subprocess.run([sys.executable, "-m", "mipipe.train.task"] + args, env=env,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return json.loads(mfile.read_text())


def test_task_eval_metrics_full_hip_graph(tmp_path):
    top1 = _task(tmp_path, "top1")
    full = _task(tmp_path, "full", "--eval-metrics", "full", "--eval-report",
                 str(tmp_path / "report.json"))
    assert full["hip_graph"] and top1["hip_graph"]
    assert full["accuracy"] == top1["accuracy"]
    assert set(full) - set(top1) == {"accuracy_top5", "eval_loss", "ece", "macro_f1",
                                     "balanced_accuracy"}
    rep = json.loads((tmp_path / "report.json").read_text())
    assert rep["rows"] == 256 and sum(sum(r) for r in rep["confusion"]) == 256
