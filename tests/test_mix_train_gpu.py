"""Mixup / CutMix in the training step on the MI355X: ResNet-18, 32 x 32, batch 8, 10 classes,
deterministic mode, 4 steps whose descriptors include an unmixed step, a Mixup and a CutMix step.

(a) the ``batch_mix`` kernel inside a step gives the bits of the same steps mixed by
    ``_ref.batch_mix``; (b) a captured step with the descriptor as its third input follows the
descriptor step by step, bit for bit like eager; (c) with the flags off the trainer is the
trainer without the feature."""
import copy
import functools
import importlib.abc
import json
import sys

import pytest
import torch

from mipipe.models import create_model
from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops.functional import cross_entropy_mixed
from mipipe.optim import SGD

pytestmark = pytest.mark.gpu

SEED, STEPS, B, HW = 12, 4, 8, 32
OPTS = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.7)
EPS = 0.1


@pytest.fixture(autouse=True)
def _deterministic():
    from mipipe.ops import determinism
    from mipipe.ops._native import load_error, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"
    determinism.set_deterministic(True)
    yield
    determinism.set_deterministic(False)


def _mixer():
    from mipipe.data.mix import BatchMixer
    return BatchMixer(SEED, 0, "cuda", **OPTS)


def test_the_steps_cover_every_mode():
    m = _mixer()
    ps = [m.params(0, s, HW, HW) for s in range(STEPS)]
    assert {int(p[1]) for p in ps} == {0, 1, 2}
    assert all(p.tobytes() != ps[0].tobytes() for p in ps[1:])
    assert all((p[3] - p[2]) * (p[5] - p[4]) > 0 for p in ps if p[1] == 2)


@functools.lru_cache(maxsize=None)
def _setup():
    torch.manual_seed(0)
    model = create_model("resnet18", num_classes=10).cuda()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(B, 3, HW, HW, generator=g).cuda() for _ in range(STEPS)]
    ys = [torch.randint(0, 10, (B,), generator=g).cuda() for _ in range(STEPS)]
    return model, xs, ys


def _train(mix_fn, frozen=False):
    """4 eager steps; ``mix_fn(x, mix)`` mixes out of place.  -> (losses, parameters)"""
    base, xs, ys = _setup()
    model = copy.deepcopy(base)
    opt = SGD(model.parameters(), 0.05, momentum=0.9, weight_decay=1e-4)
    mixer = _mixer()
    losses = []
    for s in range(STEPS):
        mix = mixer.descriptor(0, 0 if frozen else s, HW, HW)
        opt.zero_grad()
        loss = cross_entropy_mixed(model(mix_fn(xs[s], mix)), ys[s], mix, EPS)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, [p.detach().clone() for p in model.parameters()]


@functools.lru_cache(maxsize=None)
def _eager():
    return _train(lambda x, mix: K.batch_mix(x, mix))


def test_kernel_mix_equals_reference_mix_in_training():
    la, pa = _eager()
    lb, pb = _train(lambda x, mix: _ref.batch_mix(x, mix))
    assert la == lb, (la, lb)
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))
    assert all(v == v and v > 0 for v in la)


def test_graphed_step_follows_the_descriptor():
    from mipipe.train.graph import GraphedStep, graph_safe
    la, pa = _eager()
    base, xs, ys = _setup()
    model = copy.deepcopy(base)
    opt = SGD(model.parameters(), 0.05, momentum=0.9, weight_decay=1e-4)
    assert graph_safe(model, opt)[0]
    mixer = _mixer()

    def step(x, y, mix):
        opt.zero_grad()
        K.batch_mix(x, mix, out=x)  # the static input buffer, in place
        loss = cross_entropy_mixed(model(x), y, mix, EPS)
        loss.backward()
        opt.step()
        return loss

    gs = GraphedStep(step, (xs[0], ys[0], mixer.descriptor(0, 0, HW, HW)), warmup=1)
    lg = [gs.warmup_loss.item()]  # the eager warm-up trained step 0
    for s in range(1, STEPS):
        lg.append(gs.step(xs[s], ys[s], mixer.descriptor(0, s, HW, HW)).item())
    torch.cuda.synchronize()
    assert lg == la, (lg, la)
    for p, q in zip(model.parameters(), pa):
        assert torch.equal(p, q)
    # a step whose lambda and box were constants of the capture would give these instead
    lf, _ = _train(lambda x, mix: K.batch_mix(x, mix), frozen=True)
    assert lf[0] == lg[0] and all(a != b for a, b in zip(lf[1:], lg[1:])), (lf, lg)


class _NoMixImport(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path=None, target=None):
        if name == "mipipe.data.mix":
            raise ImportError("mipipe.data.mix imported with every mix flag off")
        return None


def _task(tmp_path, name, extra):
    import mipipe.train.task as T
    out = tmp_path / name
    rc = T.main(["--arch", "resnet18", "--num_classes", "10", "--dataset", "cifar10",
                 "--batch_size", str(B), "--train-samples", str(B * STEPS), "--test-samples", "16",
                 "--num_epochs", "1", "--local_training", "--model_dir", str(out),
                 "--log-every", "1", "--gpu", "0", "--metrics-file", str(out / "m.json")] + extra)
    assert rc == 0
    metrics = json.loads((out / "m.json").read_text())
    sd = torch.load(out / "resnet_distributed.pth", weights_only=True)
    return metrics, sd


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_trainer_with_the_flags_off_is_unchanged(tmp_path, monkeypatch):
    """Flags off: ``mipipe.data.mix`` is not even imported.  The same run through the new path
    with every step unmixed (``--mix-prob 0``: mode 0, lambda 1) gives the same bits, so the new
    path's identity case is the old step."""
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    saved = sys.modules.pop("mipipe.data.mix", None)
    blocker = _NoMixImport()
    sys.meta_path.insert(0, blocker)
    try:
        m0, sd0 = _task(tmp_path, "off", [])
        assert "mipipe.data.mix" not in sys.modules
    finally:
        sys.meta_path.remove(blocker)
        if saved is not None:
            sys.modules["mipipe.data.mix"] = saved
    assert "mix_lambda" not in m0 and m0["steps"] == STEPS
    m1, sd1 = _task(tmp_path, "unmixed", ["--mixup-alpha", "0.2", "--mix-prob", "0"])
    assert m1["mix_mode"] == 0 and m1["mix_lambda"] == 1.0
    assert m1["loss"] == m0["loss"], (m0["loss"], m1["loss"])
    assert _same(sd0, sd1)


def test_trainer_hip_graph_with_mixing_matches_eager(tmp_path, monkeypatch):
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    flags = ["--mixup-alpha", "0.8", "--cutmix-alpha", "1.0", "--label-smoothing", "0.1",
             "--random_seed", str(SEED), "--mix-prob", "0.7"]
    me, sde = _task(tmp_path, "eager", flags)
    mg, sdg = _task(tmp_path, "graph", flags + ["--hip-graph"])
    assert mg["hip_graph"] and not me["hip_graph"]
    assert me["mix_mode"] == mg["mix_mode"] == 2 and me["mix_lambda"] == mg["mix_lambda"]
    assert me["loss"] == mg["loss"], (me["loss"], mg["loss"])
    assert _same(sde, sdg)
    # mixing changed the run
    m0, _ = _task(tmp_path, "plain", ["--random_seed", str(SEED)])
    assert m0["loss"] != me["loss"]
