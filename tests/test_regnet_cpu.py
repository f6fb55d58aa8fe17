"""RegNet X / Y on the CPU: registry, torchvision's parameter counts and state_dict layout, the
grouped 3x3 reference ops against float64 autograd, float64 model vs reference_forward and a
task.py step."""
import pytest
import torch
import torch.nn.functional as F

from mipipe.models import create_model, model_names
from mipipe.ops import _ref

PARAMS = {"y_400mf": 4344144, "y_800mf": 6432512, "y_1_6gf": 11202430, "y_3_2gf": 19436338,
          "y_8gf": 39381472, "y_16gf": 83590140, "y_32gf": 145046770, "y_128gf": 644812894,
          "x_400mf": 5495976, "x_800mf": 7259656, "x_1_6gf": 9190136, "x_3_2gf": 15296552,
          "x_8gf": 39572648, "x_16gf": 54278536, "x_32gf": 107811560}


def test_registered_and_sorted():
    names = model_names()
    assert {f"regnet_{n}" for n in PARAMS} | {"regnet_x_nano", "regnet_y_nano"} <= set(names)
    assert names == sorted(names)


@pytest.mark.parametrize("name,count", list(PARAMS.items()))
def test_parameter_counts(name, count):
    with torch.device("meta"):
        m = create_model(f"regnet_{name}")
    assert sum(p.numel() for p in m.parameters()) == count


def test_state_dict_layout():
    y = create_model("regnet_y_400mf").state_dict()
    x = create_model("regnet_x_3_2gf").state_dict()
    want_y = {"stem.0.weight": (32, 3, 3, 3), "stem.1.running_var": (32,),
              "trunk_output.block1.block1-0.proj.0.weight": (48, 32, 1, 1),
              "trunk_output.block1.block1-0.f.a.0.weight": (48, 32, 1, 1),
              "trunk_output.block1.block1-0.f.b.0.weight": (48, 8, 3, 3),
              "trunk_output.block1.block1-0.f.se.fc1.weight": (8, 48, 1, 1),
              "trunk_output.block2.block2-0.f.se.fc1.bias": (12,),
              "trunk_output.block2.block2-2.f.se.fc2.weight": (104, 26, 1, 1),
              "trunk_output.block4.block4-5.f.c.1.weight": (440,), "fc.weight": (1000, 440)}
    want_x = {"trunk_output.block3.block3-14.f.b.0.weight": (432, 48, 3, 3),
              "trunk_output.block2.block2-0.proj.1.bias": (192,), "fc.bias": (1000,)}
    for sd, want in ((y, want_y), (x, want_x)):
        for k, shape in want.items():
            assert tuple(sd[k].shape) == shape, k
    assert not any(".se." in k for k in x) and "trunk_output.block2.block2-1.proj.0.weight" not in y


@pytest.mark.parametrize("s,G,groups,H,W", [(1, 8, 3, 5, 6), (2, 24, 2, 7, 4)])
def test_ref_ops_match_float64_autograd(s, G, groups, H, W):
    torch.manual_seed(3)
    C = G * groups
    x = torch.randn(2, H, W, C, dtype=torch.float64)
    w = torch.randn(C, 3, 3, G, dtype=torch.float64)
    shift = torch.randn(C, dtype=torch.float64)
    xr, wr = x.permute(0, 3, 1, 2).requires_grad_(True), w.permute(0, 3, 1, 2).requires_grad_(True)
    ry = F.conv2d(xr, wr, None, stride=s, padding=1, groups=groups)
    dy = torch.randn(ry.shape, dtype=torch.float64).permute(0, 2, 3, 1).contiguous()
    rdx, rdw = torch.autograd.grad(ry, (xr, wr), dy.permute(0, 3, 1, 2))
    y, ps, pss = _ref.gconv3_fwd(x, w, s, shift)
    v = y.reshape(-1, C) - shift
    add = torch.randn_like(x)
    assert torch.allclose(y, ry.detach().permute(0, 2, 3, 1), atol=1e-12)
    assert torch.allclose(ps, v.sum(0, keepdim=True)) and torch.allclose(pss, (v * v).sum(0, keepdim=True))
    assert torch.allclose(_ref.gconv3_dgrad(dy, w, x.shape, s, add), rdx.permute(0, 2, 3, 1) + add,
                          atol=1e-12)
    assert torch.allclose(_ref.gconv3_wgrad(dy, x, G, s), rdw, atol=1e-12)
    with pytest.raises(ValueError):
        _ref.gconv3_fwd(x, w, 3)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", ["regnet_x_nano", "regnet_y_nano"])
def test_forward_matches_reference_fp64(name, train):
    torch.manual_seed(11)
    m = create_model(name, num_classes=10, compute_dtype=torch.float64).double()
    x = torch.randn(4, 3, 32, 32, dtype=torch.float64)
    if not train:
        m(x)
        m.eval()
    r = __import__("copy").deepcopy(m)
    y, yr = m(x), r.reference_forward(x)
    y.square().sum().backward()
    yr.square().sum().backward()
    assert y.shape == (4, 10) and float(y.detach().abs().max()) > 0
    assert float((y - yr).detach().abs().max() / yr.detach().abs().max()) < 1e-9
    scale = max(float(p.grad.abs().max()) for p in r.parameters())
    for (n, p), q in zip(m.named_parameters(), r.parameters()):
        assert float((p.grad - q.grad).abs().max()) < 1e-9 * scale, n
    for (n, a), b in zip(m.named_buffers(), r.buffers()):
        assert float((a.double() - b.double()).abs().max()) < 1e-9, n


def test_task_runs_a_step(tmp_path, monkeypatch):
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = ["--arch", "regnet_y_nano", "--dataset", "cifar10", "--batch_size", "8",
            "--train-samples", "8", "--test-samples", "8", "--num_classes", "10",
            "--local_training", "--model_dir", str(tmp_path / "out"), "--num_epochs", "1",
            "--log-every", "0", "--metrics-file", str(tmp_path / "m.json")]
    assert T.main(args) == 0
