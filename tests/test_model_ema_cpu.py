"""Weight EMA (mipipe.optim.ModelEMA): the fp32 reference against float64, the warm-up weight,
ModelEMA on the CPU path, and task.py's flags, export and resume.  No GPU needed.
"""
import json
import math

import numpy as np
import pytest
import torch

from mipipe.ops import _ref
from mipipe.optim import SGD, ModelEMA

EPS = 2.0 ** -24  # unit roundoff of fp32


def _weights(decay, n, warmup=True, every=1):
    w_min = float(torch.tensor(1.0 - decay, dtype=torch.float64).float())
    return [_ref.ema_weight(t, every, w_min, warmup) for t in range(1, n + 1)]


def test_ref_update_against_float64():
    """50 updates of ``_ref.ema_update`` against the float64 recurrence with the same (fp32) weights.

    Bound.  One update computes ``e' = fl(e + fl(w·fl(p − e)))``: with ``|δi| <= EPS``,
    ``e' = (e + w(p − e)(1 + δ1)(1 + δ2))(1 + δ3)``, so given the same ``e`` it differs from the
    exact ``e + w(p − e)`` by at most ``EPS·(2w|p − e| + |e'|)`` to first order.  With
    ``|p| <= M`` every average is a convex combination of values in [−M, M]: ``|p − e| <= 2M``,
    ``|e'| <= M`` and, ``w <= 1``, the local error is at most ``5·EPS·M``.  An error already in
    ``e`` is multiplied by ``1 − w <= 1``, so after K updates the total is at most ``5·K·EPS·M``;
    the factor 1.01 covers the second-order terms (K·EPS ~ 3e-6)."""
    K = 50
    g = torch.Generator().manual_seed(0)
    ps = [torch.randn(4096, generator=g) for _ in range(K + 1)]
    M = max(float(p.abs().max()) for p in ps)
    for decay, warmup in ((0.9, True), (0.99998, True), (0.9, False)):
        ws = _weights(decay, K, warmup)
        e32, e64 = ps[0].clone(), ps[0].double()
        for p, w in zip(ps[1:], ws):
            _ref.ema_update(e32, p, w)
            e64 = e64 + w.double() * (p.double() - e64)
        err = float((e32.double() - e64).abs().max())
        print(decay, warmup, "max abs err", err, "bound", 5 * K * EPS * M * 1.01)
        assert err <= 5 * K * EPS * M * 1.01


def test_weight_formula():
    """max(float32(1−d), float32(9)/float32(10+u)) is 1 − min(d, (1+u)/(10+u)) to one fp32
    rounding (either branch is a single correctly rounded fp32 value of the exact one), for
    u = 0..200, and the warm-up ends where 9/(10+u) <= 1−d: u = 80 for d = 0.9, beyond the range
    for the others."""
    for d in (0.9, 0.999, 0.99998):
        w_min = np.float32(1.0 - d)
        ws = _weights(d, 201)
        first_min = None
        for u, w in enumerate(ws):
            want32 = max(w_min, np.float32(9) / np.float32(10 + u))
            assert np.float32(w.item()).view(np.uint32) == np.float32(want32).view(np.uint32)
            exact = 1.0 - min(d, (1.0 + u) / (10.0 + u))
            assert abs(float(w) - exact) <= EPS * exact * 1.001, (d, u)
            if first_min is None and float(w) == float(w_min):
                first_min = u
        assert first_min == (80 if d == 0.9 else None)
    # no warm-up: the constant; skipped calls: None
    assert all(float(w) == float(np.float32(1.0 - 0.999)) for w in _weights(0.999, 5, warmup=False))
    got = _weights(0.9, 7, every=3)
    assert [w is not None for w in got] == [False, False, True, False, False, True, False]
    assert float(got[2]) == float(np.float32(0.9)) and float(got[5]) == float(
        np.float32(9) / np.float32(11))


class SmallCNN(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 5, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(5)
        self.fc = torch.nn.Linear(5, 4)

    def forward(self, x):
        return self.fc(torch.relu(self.bn(self.conv(x))).mean((2, 3)))


def _train_step(model, opt, seed):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(6, 3, 8, 8, generator=g), torch.randint(0, 4, (6,), generator=g)
    opt.zero_grad()
    torch.nn.functional.cross_entropy(model(x), y).backward()
    opt.step()


def _snapshot(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def test_model_ema_cpu_small_cnn():
    torch.manual_seed(0)
    model = SmallCNN()
    with pytest.raises(RuntimeError, match="FlatParamSpace"):
        ModelEMA(model)  # no optimizer yet: the parameters are in no flat space
    opt = SGD(model.parameters(), lr=0.1, momentum=0.9)
    with pytest.raises(TypeError, match="DataParallel"):
        ModelEMA(torch.nn.DataParallel(model))
    ema = ModelEMA(model, decay=0.9, every=3, warmup=True)
    keys = list(model.state_dict())
    assert list(ema.module_state_dict()) == keys

    # every=3: the average moves at calls 3 and 6 only, by the reference rule
    want = {k: v.clone() for k, v in ema.module_state_dict().items()}
    for call in range(1, 8):
        _train_step(model, opt, call)
        before = ema.module_state_dict()
        ema.update()
        after = ema.module_state_dict()
        w = _ref.ema_weight(call, 3, np.float32(1.0 - 0.9), True)
        changed = any(not torch.equal(before[k], after[k]) for k in keys
                      if before[k].is_floating_point())
        assert changed == (call in (3, 6)), call
        if w is not None:
            live = model.state_dict()
            for k in keys:
                if want[k].is_floating_point():
                    _ref.ema_update(want[k], live[k], w)
            assert float(ema.last_weight()) == float(w)
        for k in keys:
            if want[k].is_floating_point():
                assert torch.equal(after[k], want[k]), (call, k)
    assert ema.num_calls() == 7 and ema.num_updates() == 2
    # integer buffers are the live ones, never averaged
    assert int(model.bn.num_batches_tracked) == 7
    assert int(ema.module_state_dict()["bn.num_batches_tracked"]) == 7

    # swapped(): the model holds the average, then everything is restored bitwise
    live, avg = _snapshot(model), ema.module_state_dict()
    flat0 = opt.space.flat.clone()
    with ema.swapped():
        inside = _snapshot(model)
        for k in keys:
            assert torch.equal(inside[k], avg[k]), k
        assert int(model.bn.num_batches_tracked) == 7
        with pytest.raises(RuntimeError, match="already active"):
            with ema.swapped():
                pass
        with pytest.raises(RuntimeError, match="swapped"):
            ema.state_dict()
    for k in keys:
        assert torch.equal(model.state_dict()[k], live[k]), k
        assert torch.equal(ema.module_state_dict()[k], avg[k]), k
    assert torch.equal(opt.space.flat, flat0)

    # state_dict round trip (weights_only-loadable) into a fresh EMA of a fresh model
    sd = ema.state_dict()
    assert sd["calls"] == 7 and sd["decay"] == 0.9 and sd["every"] == 3 and sd["warmup"] is True
    assert list(sd["model"]) == keys

    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd2 = torch.load(buf, weights_only=True)
    torch.manual_seed(1)
    m2 = SmallCNN()
    o2 = SGD(m2.parameters(), lr=0.1, momentum=0.9)
    e2 = ModelEMA(m2, decay=0.5, every=1, warmup=False)
    e2.load_state_dict(sd2)
    assert (e2.decay, e2.every, e2.warmup, e2.num_calls()) == (0.9, 3, True, 7)
    for k in keys:
        if avg[k].is_floating_point():
            assert torch.equal(e2.module_state_dict()[k], avg[k]), k
    # the loaded average continues like the original: same weights into the same next update
    assert o2.space is e2.space
    for call in (8, 9):
        _train_step(model, opt, call)
        m2.load_state_dict(model.state_dict())
        ema.update()
        e2.update()
    for k in keys:
        assert torch.equal(e2.module_state_dict()[k], ema.module_state_dict()[k]), k
    assert ema.num_updates() == 3

    # reset(): in place, back to the live weights
    ptr = ema.ema.data_ptr()
    ema.reset()
    assert ema.ema.data_ptr() == ptr and ema.num_calls() == 0
    for k in keys:
        assert torch.equal(ema.module_state_dict()[k], model.state_dict()[k]), k


TASK_ARGS = ["--arch", "mnist_cnn", "--dataset", "mnist", "--batch_size", "16", "--train-samples",
             "96", "--test-samples", "32", "--local_training", "--learning_rate", "0.05",
             "--log-every", "0", "--steps", "6"]
EMA_ARGS = ["--model-ema-decay", "0.9", "--model-ema-steps", "2"]


def _run_task(T, out, extra):
    mf = out / "m.json"
    assert T.main(TASK_ARGS + ["--model_dir", str(out), "--metrics-file", str(mf)] + extra) == 0
    return json.loads(mf.read_text())


def test_task_model_ema(tmp_path, monkeypatch):
    from mipipe.models import create_model
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = tmp_path / "a"
    m = _run_task(T, a, EMA_ARGS + ["--num_epochs", "1"])
    assert m["steps"] == 6 and m["ema_updates"] == 3
    assert 0.0 <= m["accuracy_ema"] <= 1.0 and math.isfinite(m["accuracy"])
    live = torch.load(a / "resnet_distributed.pth", weights_only=True)
    avg = torch.load(a / "resnet_distributed_ema.pth", weights_only=True)
    assert list(avg) == list(live)
    assert any(not torch.equal(avg[k], live[k]) for k in live if live[k].is_floating_point())
    create_model("mnist_cnn", num_classes=10, in_chans=1).load_state_dict(avg)
    ck = torch.load(a / "checkpoint.pth.tar", weights_only=True)
    assert ck["model_ema"]["calls"] == 6 and ck["model_ema"]["every"] == 2
    for k in avg:
        assert torch.equal(ck["model_ema"]["model"][k], avg[k]), k

    # two epochs straight == one epoch, then --resume for the second
    b = tmp_path / "b"
    m2 = _run_task(T, b, EMA_ARGS + ["--num_epochs", "2"])
    assert m2["ema_updates"] == 6
    m3 = _run_task(T, a, EMA_ARGS + ["--num_epochs", "2", "--resume"])
    assert m3["ema_updates"] == 6 and m3["accuracy_ema"] == m2["accuracy_ema"]
    s = torch.load(b / "resnet_distributed_ema.pth", weights_only=True)
    r = torch.load(a / "resnet_distributed_ema.pth", weights_only=True)
    for k in s:
        assert torch.equal(s[k], r[k]), k

    # off (the default): no second file, no new metrics key
    c = tmp_path / "c"
    m4 = _run_task(T, c, ["--num_epochs", "1"])
    assert "accuracy_ema" not in m4 and "ema_updates" not in m4
    assert (c / "resnet_distributed.pth").exists()
    assert not (c / "resnet_distributed_ema.pth").exists()
    assert "model_ema" not in torch.load(c / "checkpoint.pth.tar", weights_only=True)
    # a checkpoint without the key: the average starts from the loaded weights
    m5 = _run_task(T, c, EMA_ARGS + ["--num_epochs", "2", "--resume"])
    assert m5["ema_updates"] == 3
