"""MobileNetV3 (large / small) on the CPU: registry, torchvision's parameter counts and state-dict
layout, float64 parity of the kernel-contract path with the plain-torch reference, and a short
task.py run."""
import copy
import json

import pytest
import torch

from mipipe.models import create_model, model_names

# torchvision's published figures at 1000 classes (torchvision is not a dependency)
PARAMS = {"mobilenet_v3_large": 5_483_032, "mobilenet_v3_small": 2_542_856}
SHAPES = {
    "mobilenet_v3_large": {"features.0.0.weight": (16, 3, 3, 3),
                           "features.4.block.2.fc1.weight": (24, 72, 1, 1),
                           "features.4.block.2.fc2.bias": (72,),
                           "features.16.0.weight": (960, 160, 1, 1),
                           "classifier.3.weight": (1000, 1280)},
    "mobilenet_v3_small": {"features.0.0.weight": (16, 3, 3, 3),
                           "features.1.block.1.fc1.weight": (8, 16, 1, 1),
                           "features.12.1.running_var": (576,),
                           "classifier.0.weight": (1024, 576)},
}


@pytest.mark.parametrize("arch", sorted(PARAMS))
def test_registered_with_torchvision_layout(arch):
    assert arch in model_names()
    m = create_model(arch)
    assert sum(p.numel() for p in m.parameters()) == PARAMS[arch]
    sd = m.state_dict()
    for k, shp in SHAPES[arch].items():
        assert tuple(sd[k].shape) == shp, k
    bn = m.features[0][1]
    assert bn.eps == 1e-3 and bn.momentum == 0.01
    assert float(m.classifier[3].bias.detach().abs().max()) == 0
    assert 0.005 < float(m.classifier[3].weight.detach().std()) < 0.02


def test_constructor_arguments():
    with pytest.raises(NotImplementedError):
        create_model("mobilenet_v3_large", dilated=True)
    m = create_model("mobilenet_v3_small", num_classes=7, width_mult=0.5, reduced_tail=True,
                     dropout=0.1)
    assert m.classifier[3].out_features == 7 and m.classifier[2].p == 0.1
    full = create_model("mobilenet_v3_small", num_classes=7)
    assert sum(p.numel() for p in m.parameters()) < sum(p.numel() for p in full.parameters())
    assert all(p.shape[0] % 8 == 0 for n, p in m.named_parameters()
               if n.startswith("features") and p.dim() == 4)


@pytest.mark.parametrize("arch", sorted(PARAMS))
def test_fp64_parity_with_torch(arch):
    """The form and bounds of test_zoo_cpu.py::test_fp64_parity_with_torch, at 32 x 32."""
    torch.manual_seed(0)
    m = create_model(arch, num_classes=10, compute_dtype=torch.float64, dropout=0.0).double()
    r = copy.deepcopy(m)
    x = torch.randn(2, 3, 32, 32, dtype=torch.float64)
    a, b = m(x), r.reference_forward(x)
    assert (a - b).abs().max() <= 1e-7 * max(1.0, b.abs().max().item())
    w = torch.randn_like(a)
    (a * w).sum().backward()
    (b * w).sum().backward()
    scale = max(q.grad.abs().max().item() for q in r.parameters())
    for (n, p), (_, q) in zip(m.named_parameters(), r.named_parameters()):
        assert p.grad is not None, n
        assert (p.grad - q.grad).abs().max() <= 1e-6 * scale, n
    se = [n for n, _ in m.named_parameters() if ".fc1." in n or ".fc2." in n]
    assert se and all(float(dict(m.named_parameters())[n].grad.abs().max()) > 0 for n in se)
    for (n, bb), (_, c) in zip(m.named_buffers(), r.named_buffers()):
        assert torch.allclose(bb.double(), c.double(), rtol=1e-7, atol=1e-9), n
    m.eval()
    r.eval()
    a, b = m(x), r.reference_forward(x)
    assert (a - b).abs().max() <= 1e-7 * max(1.0, b.abs().max().item())


def test_task_trains_mobilenet_v3_small_on_cpu(tmp_path, monkeypatch):
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = ["--arch", "mobilenet_v3_small", "--dataset", "cifar10", "--batch_size", "8",
            "--train-samples", "16", "--test-samples", "8", "--num_classes", "10",
            "--local_training", "--model_dir", str(tmp_path / "out"), "--num_epochs", "1",
            "--log-every", "0", "--metrics-file", str(tmp_path / "m.json")]
    assert T.main(args) == 0
    assert json.loads((tmp_path / "m.json").read_text())["steps"] == 2
