"""Fused evaluation (mipipe.ops.inference) on the CPU reference path: the contracts of
``conv_fwd_infer`` / ``bn_fold_affine``, model parity in float64 with the switch on, the gating
of the fused path and task.py's ``--fused-eval``."""
import copy
import json

import pytest
import torch
import torch.nn.functional as F

from mipipe import nn as mnn
from mipipe.models import create_model
from mipipe.models.reference import RefVGG, ref_resnet
from mipipe.ops import _ref
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K
from mipipe.ops.inference import fused_eval, is_fused_eval, set_fused_eval


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("stride,pad", [(1, 1), (2, 1), (1, (0, 1))])
def test_ref_conv_fwd_infer_is_the_composition(stride, pad):
    torch.manual_seed(0)
    x = torch.randn(3, 9, 7, 8, dtype=torch.float64)           # NHWC
    w = torch.randn(16, 3, 3, 8, dtype=torch.float64) / 8.5    # [Co, KH, KW, Ci], unit-scale output
    scale = torch.randn(16, dtype=torch.float64)                # mixed signs
    assert (scale < 0).any() and (scale > 0).any()
    shift = torch.randn(16, dtype=torch.float64) * 0.5
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad)
    res = torch.randn_like(_nhwc(y))
    for sc, sh, r, relu in [(scale, shift, res, True), (scale, shift, None, True),
                            (None, None, res, False), (None, None, None, False),
                            (scale, None, res, True), (None, shift, None, False)]:
        ref = y
        if sc is not None:
            ref = ref * sc[None, :, None, None]
        if sh is not None:
            ref = ref + sh[None, :, None, None]
        ref = _nhwc(ref)
        if r is not None:
            ref = ref + r
        if relu:
            ref = torch.relu(ref)
        out = _ref.conv_fwd_infer(x, w, stride, pad, sc, sh, r, relu)
        assert out.dtype == torch.float64
        assert (out - ref).abs().max() <= 1e-12
        # the dispatcher takes the same route on CPU tensors
        assert torch.equal(K.conv_fwd_infer(x, w, stride, pad, sc, sh, r, relu), out)


@pytest.mark.parametrize("with_bias", [False, True])
def test_ref_bn_fold_affine_is_eval_batchnorm(with_bias):
    torch.manual_seed(1)
    C = 24
    y = torch.randn(2, C, 5, 6, dtype=torch.float64)
    gamma = torch.rand(C, dtype=torch.float64) + 0.5
    beta = torch.randn(C, dtype=torch.float64) * 0.1
    mean = torch.randn(C, dtype=torch.float64)
    var = torch.rand(C, dtype=torch.float64) + 0.3
    cb = torch.randn(C, dtype=torch.float64) if with_bias else None
    eps = 1e-5
    yb = y if cb is None else y + cb[None, :, None, None]
    ref = F.batch_norm(yb, mean, var, gamma, beta, training=False, eps=eps)
    scale, shift = _ref.bn_fold_affine(gamma, beta, mean, var, eps, cb)
    assert scale.dtype == shift.dtype == torch.float64
    out = y * scale[None, :, None, None] + shift[None, :, None, None]
    assert (out - ref).abs().max() <= 1e-12
    s2, h2 = K.bn_fold_affine(gamma, beta, mean, var, eps, cb)
    assert torch.equal(s2, scale) and torch.equal(h2, shift)


def _settle_bn(m, x, steps=3):
    """Running statistics of the data, then random affine parameters."""
    m.train()
    with torch.no_grad():
        for _ in range(steps):
            m(x)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0.0, 0.1)
    m.eval()


def test_resnet18_fused_eval_fp64():
    torch.manual_seed(0)
    m = create_model("resnet18", num_classes=10, compute_dtype=torch.float64).double()
    x = torch.randn(4, 3, 32, 32, dtype=torch.float64)
    _settle_bn(m, x)
    r = ref_resnet("resnet18", num_classes=10).double().eval()
    r.load_state_dict(m.state_dict())
    with torch.no_grad():
        ref = r(x)
        with fused_eval():
            assert is_fused_eval()
            fused = m(x)
        assert not is_fused_eval()
        plain = m(x)
    assert (fused - ref).abs().max() < 1e-9
    assert (plain - fused).abs().max() < 1e-9


@pytest.mark.parametrize("arch,kw,res", [("resnet50", {}, 64), ("vgg11_bn", dict(dropout=0.0), 32),
                                         ("mobilenet_v2", dict(dropout=0.0), 32)])
def test_architectures_fused_eval_fp64(arch, kw, res, monkeypatch):
    torch.manual_seed(0)
    m = create_model(arch, num_classes=10, **kw).double()
    m.compute_dtype = torch.float64
    x = torch.randn(2, 3, res, res, dtype=torch.float64)
    _settle_bn(m, x)
    if arch.startswith("resnet"):
        r = ref_resnet(arch, num_classes=10).double().eval()
        r.load_state_dict(m.state_dict())
        ref_fwd = r.forward
    elif arch.startswith("vgg"):
        r = RefVGG(arch, num_classes=10, dropout=0.0).double().eval()
        r.load_state_dict(m.state_dict())
        ref_fwd = r.forward
    else:
        ref_fwd = copy.deepcopy(m).reference_forward
    calls = []
    real = K.conv_fwd_infer
    monkeypatch.setattr(K, "conv_fwd_infer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        ref = ref_fwd(x)
        with fused_eval():
            out = m(x)
    assert calls, "the fused path was not taken"
    assert (out - ref).abs().max() <= 1e-7 * max(1.0, ref.abs().max().item())


def test_gating(monkeypatch):
    torch.manual_seed(0)
    m = create_model("resnet18", num_classes=10)
    x = torch.randn(2, 3, 32, 32)

    def boom(*a, **k):
        raise AssertionError("conv_fwd_infer reached")

    monkeypatch.setattr(K, "conv_fwd_infer", boom)
    m.eval()
    with torch.no_grad():          # switch off
        m(x)
    with fused_eval():
        m(x)                       # eval, but grad enabled
        m.train()
        with torch.no_grad():      # training mode
            m(x)
        m(x)
    # switch on, eval, no_grad: one fused launch per conv outside the stem, no BN-apply pass
    m.eval()
    n_convs = sum(isinstance(mod, mnn.Conv2d) for mod in m.modules()) - 1
    n_down = sum(1 for n, mod in m.named_modules() if n.endswith("downsample.0"))
    assert (n_convs, n_down) == (19, 3)   # 16 basic-block convs + 3 downsample convs
    calls = []
    monkeypatch.setattr(K, "conv_fwd_infer",
                        lambda *a, **k: (calls.append(1), _ref.conv_fwd_infer(*a, **k))[1])

    def no_bn_act(*a, **k):
        raise AssertionError("bn_act_fwd reached on the fused path")

    with torch.no_grad(), fused_eval():
        m(x)
        assert len(calls) == n_convs
        # (the stem keeps its own path — conv + BN/ReLU/max-pool — so the ban starts behind it)
        h = m.conv1.pack_input(x, torch.float32)
        h = mnn.conv_bn_relu_maxpool(h, m.conv1, m.bn1, m.maxpool)
        monkeypatch.setattr(K, "bn_act_fwd", no_bn_act)
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            h = layer(h)
    assert len(calls) == 2 * n_convs


def test_conv_affine_act_is_inference_only():
    x = torch.randn(1, 4, 4, 8)
    w = torch.randn(8, 1, 1, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        MF.conv_affine_act(x, w, None, None, 1, 0, False)
    with torch.no_grad():
        y = MF.conv_affine_act(x, w, None, None, 1, 0, True)
    assert not y.requires_grad and (y >= 0).all()
    y = MF.conv_affine_act(x, w.detach(), None, None, 1, 0, False)   # nothing requires grad
    assert y.grad_fn is None


def test_switch_env_default(monkeypatch):
    import importlib
    from mipipe.ops import inference
    old = inference.is_fused_eval()
    try:
        monkeypatch.setenv("MIPIPE_FUSED_EVAL", "1")
        assert importlib.reload(inference).is_fused_eval()
        monkeypatch.delenv("MIPIPE_FUSED_EVAL")
        assert not importlib.reload(inference).is_fused_eval()
    finally:
        set_fused_eval(old)
        inference.set_fused_eval(old)


def _run_task(tmp_path, fused):
    from mipipe.train import task as T
    out = tmp_path / f"m{fused}.json"
    args = ["--arch", "resnet18", "--dataset", "cifar10", "--batch_size", "8",
            "--train-samples", "16", "--test-samples", "8", "--num_classes", "10",
            "--local_training", "--model_dir", str(tmp_path / f"out{fused}"), "--num_epochs", "1",
            "--log-every", "0", "--metrics-file", str(out), "--fused-eval", str(fused)]
    assert T.main(args) == 0
    return json.loads(out.read_text())


def test_task_fused_eval_cpu(tmp_path, monkeypatch):
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("MIPIPE_FUSED_EVAL", raising=False)
    calls = []
    real = K.conv_fwd_infer
    monkeypatch.setattr(K, "conv_fwd_infer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    off = _run_task(tmp_path, 0)
    assert not calls and off["fused_eval"] is False
    on = _run_task(tmp_path, 1)
    assert calls and on["fused_eval"] is True
    assert on["steps"] == off["steps"] == 2
    assert on["accuracy"] == off["accuracy"]
