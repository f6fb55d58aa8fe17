"""Vision Transformer family on the CPU: registry, torchvision state_dict layout, the fp32 / fp64
contracts of the new kernels, float64 parity of ``model(x)`` with ``reference_forward`` (logits and
every parameter gradient) and the ``task.py`` flags."""
import glob
import json
import math

import pytest
import torch
import torch.nn.functional as F

from mipipe.models import create_model, model_names
from mipipe.ops import _ref
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K

PARAMS = {"vit_b_16": 86_567_656, "vit_b_32": 88_224_232,
          "vit_l_16": 304_326_632, "vit_l_32": 306_535_400}


def test_registry_lists_the_family():
    names = model_names()
    for n in list(PARAMS) + ["vit_tiny"]:
        assert n in names
    assert "vit_h_14" not in names


@pytest.mark.parametrize("arch", list(PARAMS))
def test_parameter_counts(arch):
    with torch.device("meta"):
        m = create_model(arch)
    assert sum(p.numel() for p in m.parameters()) == PARAMS[arch]


def test_state_dict_keys_follow_torchvision():
    m = create_model("vit_tiny", num_classes=10)
    sd = m.state_dict()
    D, S = 256, 17
    want = ["class_token", "conv_proj.weight", "conv_proj.bias", "encoder.pos_embedding",
            "encoder.ln.weight", "encoder.ln.bias", "heads.head.weight", "heads.head.bias"]
    for i in range(2):
        pre = f"encoder.layers.encoder_layer_{i}."
        want += [pre + k for k in (
            "ln_1.weight", "ln_1.bias", "self_attention.in_proj_weight",
            "self_attention.in_proj_bias", "self_attention.out_proj.weight",
            "self_attention.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.0.weight",
            "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")]
    assert sorted(sd) == sorted(want)
    assert sd["class_token"].shape == (1, 1, D)
    assert sd["conv_proj.weight"].shape == (D, 3, 16, 16)
    assert sd["encoder.pos_embedding"].shape == (1, S, D)
    assert sd["encoder.layers.encoder_layer_0.self_attention.in_proj_weight"].shape == (3 * D, D)
    assert sd["encoder.layers.encoder_layer_1.mlp.0.weight"].shape == (512, D)
    assert sd["heads.head.weight"].shape == (10, D)


def _randomise(m, seed=1):
    """The zero-init head and class token hide errors: give them values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.heads.head.weight.copy_(torch.randn(m.heads.head.weight.shape, generator=g) * 0.1)
        m.heads.head.bias.copy_(torch.randn(m.heads.head.bias.shape, generator=g) * 0.1)
        m.class_token.copy_(torch.randn(m.class_token.shape, generator=g) * 0.1)
    return m


def test_state_dict_roundtrip_and_old_mlp_names():
    torch.manual_seed(0)
    a = _randomise(create_model("vit_tiny", num_classes=10)).eval()
    x = torch.randn(2, 3, 64, 64)
    ya = a(x)
    b = create_model("vit_tiny", num_classes=10).eval()
    b.load_state_dict(a.state_dict())
    assert torch.equal(b(x), ya)
    old = {k.replace(".mlp.0.", ".mlp.linear_1.").replace(".mlp.3.", ".mlp.linear_2."): v
           for k, v in a.state_dict().items()}
    assert any(".mlp.linear_1." in k for k in old)
    c = create_model("vit_tiny", num_classes=10).eval()
    c.load_state_dict(old)
    assert torch.equal(c(x), ya)


def test_unsupported_configurations_raise():
    from mipipe.models.vit import VisionTransformer
    with pytest.raises(ValueError, match="64"):  # vit_h_14: hidden 1280 / 16 heads = 80
        VisionTransformer(14, 2, 16, 1280, 5120)
    with pytest.raises(ValueError, match="multiple of 8"):
        VisionTransformer(14, 2, 4, 256, 512, image_size=224)
    with pytest.raises(ValueError, match="not a multiple"):
        VisionTransformer(16, 2, 4, 256, 512, image_size=72)
    m = create_model("vit_tiny", num_classes=10)
    with pytest.raises(ValueError, match="not interpolated"):
        m(torch.randn(1, 3, 96, 96))
    with pytest.raises(ValueError, match="multiple of the patch"):
        m(torch.randn(1, 3, 64, 72))
    with pytest.raises(ValueError, match="expected"):
        m(torch.randn(1, 1, 64, 64))


def test_ref_patchify_is_unfold():
    torch.manual_seed(0)
    x = torch.randn(3, 3, 32, 48)
    want = F.unfold(x, 16, stride=16).transpose(1, 2).reshape(-1, 3 * 16 * 16)
    got = _ref.patchify(x, 16, torch.float32)
    assert got.shape == (3 * 2 * 3, 768) and torch.equal(got, want)
    assert torch.equal(K.patchify(x, 16, torch.float32), want)
    # ... and the rows are the patch convolution's GEMM operand as the filter stands
    w = torch.randn(8, 3, 16, 16)
    conv = F.conv2d(x, w, stride=16).flatten(2).transpose(1, 2).reshape(-1, 8)
    torch.testing.assert_close(got @ w.view(8, -1).t(), conv, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError):
        _ref.patchify(torch.randn(1, 3, 30, 32), 16, torch.float32)


def test_ref_tokens_assemble_matches_autograd_of_cat_add():
    torch.manual_seed(0)
    B, N, D = 3, 6, 16
    e = torch.randn(B * N, D, dtype=torch.float64, requires_grad=True)
    cls = torch.randn(1, 1, D, dtype=torch.float64, requires_grad=True)
    pos = torch.randn(1, N + 1, D, dtype=torch.float64, requires_grad=True)
    want = (torch.cat([cls.expand(B, -1, -1), e.view(B, N, D)], 1) + pos).reshape(-1, D)
    got = _ref.tokens_assemble_fwd(e.detach(), cls.detach().reshape(-1), pos.detach().reshape(-1))
    assert torch.equal(got, want.detach())
    dh = torch.randn(B * (N + 1), D, dtype=torch.float64)
    ge, gc, gp = torch.autograd.grad(want, (e, cls, pos), dh)
    de, dpos, dcls = _ref.tokens_assemble_bwd(dh, B)
    assert torch.equal(de, ge)
    torch.testing.assert_close(dpos.view(1, N + 1, D), gp, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dcls.view(1, 1, D), gc, rtol=1e-12, atol=1e-12)
    # the autograd function over the same contract, accumulators included
    h = MF.tokens_assemble(e, cls, pos)
    ge2, gc2, gp2 = torch.autograd.grad(h, (e, cls, pos), dh)
    assert torch.equal(ge2, ge)
    torch.testing.assert_close(gc2, gc, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gp2, gp, rtol=1e-12, atol=1e-12)
    ap, ac = torch.ones((N + 1) * D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
    _, none_p, none_c = K.tokens_assemble_bwd(dh, B, ap, ac)
    assert none_p is None and none_c is None
    torch.testing.assert_close(ap, dpos + 1, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ac, dcls + 1, rtol=1e-12, atol=1e-12)


def test_ref_layernorm_bwd_addend():
    torch.manual_seed(0)
    R, H = 7, 32
    x, dy, ds = (torch.randn(R, H, dtype=torch.float64) for _ in range(3))
    gamma, beta = torch.rand(H, dtype=torch.float64) + 0.5, torch.randn(H, dtype=torch.float64)
    _, mean, rstd, _ = _ref.layernorm_fwd(x, gamma, beta, 1e-6)
    dx0, dg0, db0 = _ref.layernorm_bwd(dy, x, mean, rstd, gamma)
    dx1, dg1, db1 = _ref.layernorm_bwd(dy, x, mean, rstd, gamma, ds)
    assert torch.equal(dx1, dx0 + ds) and torch.equal(dg1, dg0) and torch.equal(db1, db0)
    # K.layernorm_bwd off the native path: the bias sum covers the total; dropout is refused
    dbias = torch.zeros(H, dtype=torch.float64)
    dx2, _, _, _ = K.layernorm_bwd(dy, x, mean, rstd, gamma, dbias=dbias, dsum=ds)
    assert torch.equal(dx2, dx1)
    torch.testing.assert_close(dbias, dx1.sum(0), rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match="dropout"):
        K.layernorm_bwd(dy, x, mean, rstd, gamma, drop=(0.1, 3), dsum=ds)


def test_add_layer_norm_matches_autograd():
    torch.manual_seed(0)
    R, H = 5, 32
    x, res = (torch.randn(R, H, dtype=torch.float64, requires_grad=True) for _ in range(2))
    gamma = (torch.rand(H, dtype=torch.float64) + 0.5).requires_grad_()
    beta = torch.randn(H, dtype=torch.float64, requires_grad=True)
    wy, ws = torch.randn(R, H, dtype=torch.float64), torch.randn(R, H, dtype=torch.float64)
    leaves = (x, res, gamma, beta)
    y, xs = MF.add_layer_norm(x, res, gamma, beta, 1e-6)
    s = x + res
    yr = F.layer_norm(s, (H,), gamma, beta, 1e-6)
    torch.testing.assert_close(y, yr, rtol=1e-12, atol=1e-12)
    assert torch.equal(xs, s)
    for use_y, use_s in ((True, True), (True, False), (False, True)):
        got = torch.autograd.grad((y * wy).sum() * use_y + (xs * ws).sum() * use_s, leaves,
                                  retain_graph=True, allow_unused=True)
        want = torch.autograd.grad((yr * wy).sum() * use_y + (s * ws).sum() * use_s, leaves,
                                   retain_graph=True, allow_unused=True)
        for a, b in zip(got, want):
            if b is None:
                assert a is None or not a.abs().any()
            else:
                torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("patch", [16, 32])
def test_vit_tiny_float64_matches_reference_forward(patch):
    """Image 64 with patch 16 (S = 17) and patch 32 (S = 5), B = 3: the logits and every parameter
    gradient of model(x) equal reference_forward(x) (F.conv2d, F.multi_head_attention_forward,
    F.layer_norm) to 1e-9 relative in float64."""
    torch.manual_seed(0)
    m = create_model("vit_tiny", num_classes=10, patch_size=patch,
                     compute_dtype=torch.float64).double()
    _randomise(m)
    assert m.seq_length == (64 // patch) ** 2 + 1
    x = torch.randn(3, 3, 64, 64, dtype=torch.float64)
    out, ref = m(x), m.reference_forward(x)
    assert out.shape == (3, 10)
    assert ((out - ref).abs().max() / ref.abs().max()).item() < 1e-9
    w = torch.randn(3, 10, dtype=torch.float64)
    params = list(m.parameters())
    g_out = torch.autograd.grad((out * w).sum(), params)
    g_ref = torch.autograd.grad((ref * w).sum(), params)
    for (n, _), a, b in zip(m.named_parameters(), g_out, g_ref):
        assert b.abs().max() > 0 or "in_proj_bias" in n, n
        assert ((a - b).abs().max() / (b.abs().max() + 1e-300)).item() < 1e-9, n


def _task_args(tmp_path):
    return ["--arch", "vit_tiny", "--dataset", "cifar10", "--image-size", "64", "--num_classes",
            "10", "--batch_size", "8", "--train-samples", "8", "--test-samples", "8",
            "--local_training", "--model_dir", str(tmp_path / "o"), "--learning_rate", "0.001",
            "--log-every", "1", "--log-dir", str(tmp_path / "log"), "--num_epochs", "2",
            "--optimizer", "adamw", "--wd", "0.05", "--metrics-file", str(tmp_path / "m.json")]


def test_task_vit_tiny_adamw_two_cpu_steps(tmp_path, monkeypatch):
    """Two AdamW steps over the same 8 samples (one batch per epoch): the loss goes down."""
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert T.main(_task_args(tmp_path)) == 0
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["arch"] == "vit_tiny" and m["steps"] == 2
    losses = []
    for f in glob.glob(str(tmp_path / "log" / "*")):
        for line in open(f):
            rec = json.loads(line)
            if rec.get("event") == "step":
                losses.append(rec["loss"])
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert abs(losses[0] - math.log(10)) < 1e-3  # zero-init head: uniform prediction
    assert losses[1] < losses[0], losses


@pytest.mark.parametrize("extra", [["--lr-schedule", "cosine"], ["--lr-warmup-steps", "2"],
                                   ["--clip-grad-norm", "1"]])
def test_task_adamw_refuses_schedule_and_clipping(tmp_path, monkeypatch, extra):
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match="--optimizer lamb"):
        T.main(_task_args(tmp_path) + extra)
