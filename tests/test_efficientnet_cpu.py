"""EfficientNet b0 ... b7 on the CPU: registry, torchvision's parameter counts and state_dict
layout, BatchNorm settings, the stochastic-depth schedule, float64 model vs reference_forward and
the task.py flag."""
import pytest
import torch

from mipipe.models import create_model, model_names
from mipipe.ops import kernels as K

NAMES = [f"efficientnet_b{i}" for i in range(8)]
PARAMS = [5288548, 7794184, 9109994, 12233232, 19341616, 30389784, 43040704, 66347960]


def test_registered():
    assert set(NAMES) <= set(model_names())


@pytest.mark.parametrize("name,count", list(zip(NAMES, PARAMS)))
def test_parameter_counts(name, count):
    assert sum(p.numel() for p in create_model(name).parameters()) == count


def test_state_dict_layout_and_batchnorm_settings():
    sd = create_model("efficientnet_b0").state_dict()
    want = {"features.0.0.weight": (32, 3, 3, 3), "features.1.0.block.0.0.weight": (32, 1, 3, 3),
            "features.2.0.block.1.0.weight": (96, 1, 3, 3),
            "features.2.0.block.2.fc1.weight": (4, 96, 1, 1), "features.8.1.running_var": (1280,),
            "classifier.1.weight": (1000, 1280)}
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    bn0 = create_model("efficientnet_b0").features[0][1]
    bn5 = create_model("efficientnet_b5", num_classes=10).features[0][1]
    assert (bn0.eps, bn0.momentum) == (1e-5, 0.1) and (bn5.eps, bn5.momentum) == (1e-3, 0.01)


def test_stochastic_depth_schedule():
    m = create_model("efficientnet_b0")
    assert m.stochastic_depth_prob == 0.2
    assert [b.sd_prob for b in m.blocks()] == pytest.approx([0.2 * i / 16 for i in range(16)])
    assert create_model("efficientnet_b0", stochastic_depth_prob=0.0).blocks()[-1].sd_prob == 0.0
    with pytest.raises(ValueError, match="stochastic_depth_prob"):
        create_model("efficientnet_b0", stochastic_depth_prob=1.0)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("size,depth", [(32, 0.5), (35, 1.5)])
def test_forward_matches_reference_fp64(size, depth, train):
    """A small build at 32 x 32 and at an odd-map size (35 -> 18 -> 9 -> 5 -> 3 -> 2); depth 1.5
    gives the first stage a second block, whose residual gradient goes through the depthwise
    data-grad's addend.  In training both paths apply the same keep masks."""
    torch.manual_seed(11)
    m = create_model("efficientnet_b0", width_mult=0.5, depth_mult=depth, num_classes=10,
                     dropout=0.0, stochastic_depth_prob=0.5, compute_dtype=torch.float64,
                     seed=5).double()
    m.train(train)
    x = torch.randn(4, 3, size, size, dtype=torch.float64)
    y = m(x)
    y.square().sum().backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    r = m.reference_forward(x)
    r.square().sum().backward()
    assert y.shape == (4, 10) and float(y.detach().abs().max()) > 0
    assert float((y - r).detach().abs().max() / r.detach().abs().max()) < 1e-9
    # (some gradients are zero in exact arithmetic: the scale is the model's largest, not their own)
    scale = max(float(p.grad.abs().max()) for p in m.parameters())
    for n, p in m.named_parameters():
        assert p.grad is not None and got[n] is not None, n
        assert float((got[n] - p.grad).abs().max()) < 1e-9 * scale, n
    if train:
        keeps = torch.stack([K.drop_path_keep(4, b.sd_prob, s)
                             for b, s in zip(m.blocks(), m._last_seeds) if b.sd_prob > 0])
        assert not bool(keeps.all()) and bool(keeps.any())


def test_task_stochastic_depth_flag(tmp_path, monkeypatch):
    import mipipe.train.task as T
    a = T.build_parser().parse_args(["--arch", "efficientnet_b0", "--stochastic-depth", "0.1"])
    assert a.arch == "efficientnet_b0" and a.stochastic_depth == 0.1
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    args = ["--dataset", "cifar10", "--batch_size", "8", "--train-samples", "16", "--test-samples",
            "8", "--local_training", "--model_dir", str(tmp_path / "o"), "--num_epochs", "1"]
    with pytest.raises(SystemExit, match="stochastic-depth"):
        T.main(args + ["--arch", "resnet18", "--stochastic-depth", "0.1"])
