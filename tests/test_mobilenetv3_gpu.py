"""MobileNetV3 end to end on the GPU: bf16 kernels against the fp32 plain-torch reference,
training steps, flat-buffer gradients of the SE FCs and the BatchNorms, a replayed captured step
and task.py --hip-graph.  (No model-level bit determinism is asserted: the generic depthwise
weight-grad uses float atomics; the new kernels' determinism is asserted in
test_se_kernels_gpu.py.)"""
import json
import math

import pytest
import torch

from mipipe.models import create_model
from mipipe.ops import functional as MF
from mipipe.ops._native import native_available

pytestmark = pytest.mark.gpu

dev = "cuda"
ARCHS = ["mobilenet_v3_large", "mobilenet_v3_small"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(1234)
    yield


def cos(a, b):
    """test_zoo_gpu.py's scale-invariant cosine."""
    a, b = a.flatten().double(), b.flatten().double()
    a, b = a / (a.abs().max() + 1e-300), b / (b.abs().max() + 1e-300)
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


@pytest.mark.parametrize("arch", ARCHS)
def test_eval_matches_fp32_torch(arch):
    torch.manual_seed(0)
    m = create_model(arch, num_classes=100, dropout=0.0).cuda().eval()
    x = torch.randn(4, 3, 64, 64, device=dev)
    with torch.no_grad():
        out, ref = m(x), m.reference_forward(x)
    assert out.dtype == torch.bfloat16 and out.shape == ref.shape == (4, 100)
    assert cos(out, ref) > 0.99, cos(out, ref)


@pytest.mark.parametrize("arch", ARCHS)
def test_train_steps_reduce_loss(arch):
    """As test_zoo_train_steps_reduce_loss; the flat-buffer gradients of the SE FCs and of every
    BatchNorm are non-zero and finite after the first backward."""
    from mipipe.optim import SGD
    from mipipe.train.task import CrossEntropyLoss
    torch.manual_seed(0)
    m = create_model(arch, num_classes=10).cuda()
    m.compute_dtype = torch.bfloat16
    opt = SGD(m.parameters(), 0.005, momentum=0.9, weight_decay=1e-4, shadow_dtype=torch.bfloat16)
    crit = CrossEntropyLoss()
    x = torch.randn(8, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (8,), device=dev)
    bn_names = {n + s for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)
                for s in (".weight", ".bias")}
    losses = []
    m.train()
    for step in range(5):
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        if step == 0:
            watched = 0
            for n, p in m.named_parameters():
                if ".fc1." in n or ".fc2." in n or n in bn_names:
                    watched += 1
                    assert p.grad is not None and torch.isfinite(p.grad).all(), n
                    assert float(p.grad.abs().max()) > 0, n
            assert watched > 60
        opt.step()
        losses.append(float(loss.item()))
    assert all(math.isfinite(v) for v in losses), losses
    assert min(losses[1:]) < losses[0], losses


def test_captured_step_replays():
    from mipipe.optim import SGD
    from mipipe.train.graph import GraphedStep, graph_safe
    torch.manual_seed(0)
    # (dropout off: a captured step would replay one host-seeded classifier mask, so graph_safe
    # refuses models whose Dropout is active)
    m = create_model("mobilenet_v3_small", num_classes=10, dropout=0.0).cuda()
    opt = SGD(m.parameters(), 0.01, momentum=0.9)
    ok, why = graph_safe(m, opt)
    assert ok, why
    x = torch.randn(8, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (8,), device=dev)

    def step(xx, yy):
        opt.zero_grad()
        loss = MF.cross_entropy(m(xx), yy)
        loss.backward()
        opt.step()
        return loss

    gs = GraphedStep(step, (x, y), warmup=1, inputs=[(x, y)])
    probe = m.features[4].block[2].fc1.weight
    seen = [probe.detach().clone()]
    losses = [gs.warmup_loss.item()]
    for _ in range(3):
        losses.append(gs.replay(0).item())
        torch.cuda.synchronize()
        seen.append(probe.detach().clone())
    assert all(math.isfinite(v) for v in losses), losses
    for a, b in zip(seen, seen[1:]):
        assert not torch.equal(a, b)


def test_task_hip_graph_run(tmp_path, monkeypatch):
    """task.py --hip-graph finishes: with the classifier's Dropout active (task.py builds the
    default model) it reports the capture refused and trains eagerly, as for mobilenet_v2."""
    import mipipe.train.task as T
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mfile = tmp_path / "m.json"
    rc = T.main(["--arch", "mobilenet_v3_small", "--num_classes", "10", "--dataset", "cifar10",
                 "--batch_size", "32", "--train-samples", str(32 * 3), "--test-samples", "32",
                 "--num_epochs", "1", "--local_training", "--model_dir", str(tmp_path / "out"),
                 "--log-every", "0", "--gpu", "0", "--hip-graph", "--metrics-file", str(mfile)])
    assert rc == 0
    met = json.loads(mfile.read_text())
    assert met["steps"] == 3 and math.isfinite(met["loss"])
