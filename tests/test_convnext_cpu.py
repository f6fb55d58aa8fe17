"""ConvNeXt on the CPU: registry, parameter counts, torchvision's state-dict layout, float64
parity of ``forward`` with ``reference_forward`` (with and without stochastic depth), and the
reference contracts of the new kernels against autograd of the plain torch composition."""
import pytest
import torch
import torch.nn.functional as F

from mipipe.models import create_model, model_names
from mipipe.ops import _ref
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K

FAMILY = {  # depths, widths, parameter count at 1000 classes (torchvision's figures)
    "convnext_tiny": ((3, 3, 9, 3), (96, 192, 384, 768), 28_589_128),
    "convnext_small": ((3, 3, 27, 3), (96, 192, 384, 768), 50_223_688),
    "convnext_base": ((3, 3, 27, 3), (128, 256, 512, 1024), 88_591_464),
    "convnext_large": ((3, 3, 27, 3), (192, 384, 768, 1536), 197_767_336),
}
ALL_DROPPED_SEED = 105  # written into tests/test_convnext_kernels_gpu.py


def test_registry_lists_the_family():
    names = model_names()
    for n in list(FAMILY) + ["convnext_atto"]:
        assert n in names


def _formula(depths, dims, classes=1000):
    """8C^2 + 58C per block (49C + C depthwise, 2C LayerNorm, 4C^2 + 4C and 4C^2 + C Linears, C
    layer scale), 4 Cin Cout + Cout + 2 Cin per downsample, 48 C0 + 3 C0 for the stem (conv, bias,
    LayerNorm), 2C + 1000C + 1000 for the head."""
    n = 48 * dims[0] + 3 * dims[0]
    for i, (d, c) in enumerate(zip(depths, dims)):
        n += d * (8 * c * c + 58 * c)
        if i < 3:
            n += 4 * c * dims[i + 1] + dims[i + 1] + 2 * c
    return n + 2 * dims[-1] + classes * dims[-1] + classes


@pytest.mark.parametrize("arch", list(FAMILY))
def test_parameter_counts(arch):
    depths, dims, count = FAMILY[arch]
    with torch.device("meta"):
        m = create_model(arch)
    got = sum(p.numel() for p in m.parameters())
    assert got == _formula(depths, dims) == count
    assert m.depths == depths and m.dims == dims


def test_stochastic_depth_defaults_and_schedule():
    for arch, p in (("convnext_tiny", 0.1), ("convnext_small", 0.4), ("convnext_base", 0.5),
                    ("convnext_large", 0.5)):
        with torch.device("meta"):
            m = create_model(arch)
        ps = [b.sd_prob for b in m.blocks()]
        n = len(ps)
        assert m.stochastic_depth_prob == p and ps[0] == 0.0 and ps[-1] == pytest.approx(p)
        assert ps == pytest.approx([p * i / (n - 1) for i in range(n)])
    with torch.device("meta"):
        m = create_model("convnext_tiny", stochastic_depth_prob=0.3)
    assert m.blocks()[-1].sd_prob == pytest.approx(0.3)
    with pytest.raises(ValueError, match="stochastic_depth_prob"):
        create_model("convnext_atto", stochastic_depth_prob=1.0)


def test_state_dict_layout_and_round_trip():
    m = create_model("convnext_atto", num_classes=10)
    sd = m.state_dict()
    want = {
        "features.0.0.weight": (40, 3, 4, 4), "features.0.0.bias": (40,),
        "features.0.1.weight": (40,), "features.0.1.bias": (40,),
        "features.1.0.block.0.weight": (40, 1, 7, 7), "features.1.0.block.0.bias": (40,),
        "features.1.1.block.2.weight": (40,), "features.1.1.block.2.bias": (40,),
        "features.1.0.block.3.weight": (160, 40), "features.1.0.block.3.bias": (160,),
        "features.1.0.block.5.weight": (40, 160), "features.1.0.block.5.bias": (40,),
        "features.1.0.layer_scale": (40, 1, 1),
        "features.2.0.weight": (40,), "features.2.0.bias": (40,),
        "features.2.1.weight": (80, 40, 2, 2), "features.2.1.bias": (80,),
        "features.3.1.block.0.weight": (80, 1, 7, 7),
        "features.4.1.weight": (160, 80, 2, 2),
        "features.5.5.block.5.weight": (160, 640), "features.5.5.layer_scale": (160, 1, 1),
        "features.6.0.weight": (160,), "features.6.1.bias": (320,),
        "features.7.1.block.3.weight": (1280, 320),
        "classifier.0.weight": (320,), "classifier.0.bias": (320,),
        "classifier.2.weight": (10, 320), "classifier.2.bias": (10,),
    }
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
    # 4 stem + 3 * 4 downsample + 4 head tensors, 9 per block; nothing else (no buffers)
    assert len(sd) == 4 + 12 + 4 + 9 * 12
    assert all(k.split(".")[0] in ("features", "classifier") for k in sd)
    # torchvision's initialisation
    assert torch.all(sd["features.1.0.layer_scale"] == 1e-6)
    assert not sd["classifier.2.bias"].any() and not sd["features.1.0.block.0.bias"].any()
    assert 0.015 < sd["features.5.0.block.3.weight"].std() < 0.025
    assert sd["features.5.0.block.3.weight"].abs().max() <= 2.0
    m2 = create_model("convnext_atto", num_classes=10)
    m2.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    x = torch.randn(2, 3, 32, 32)
    m.eval(), m2.eval()
    assert torch.equal(m(x), m2(x))


def _randomise(m):
    """layer_scale = 1e-6 and a zero head hide every error: re-randomise them."""
    with torch.no_grad():
        for b in m.blocks():
            b.layer_scale.uniform_(0.5, 1.5)
        m.classifier[2].weight.normal_(std=0.1)
        m.classifier[2].bias.normal_(std=0.1)
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("sd_prob", [0.0, 0.5])
@pytest.mark.parametrize("size", [32, 40])
def test_forward_matches_reference_fp64(size, sd_prob, train):
    """Maps 8 -> 4 -> 2 -> 1 (smaller than the 7x7 kernel) and 10 -> 5 -> 2 -> 1 (an odd map
    floors).  In training both paths apply the same keep masks."""
    torch.manual_seed(11)
    m = create_model("convnext_atto", num_classes=10, stochastic_depth_prob=sd_prob,
                     compute_dtype=torch.float64, seed=5).double()
    _randomise(m)
    m.train(train)
    x = torch.randn(4, 3, size, size, dtype=torch.float64)
    y = m(x)
    y.square().sum().backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    r = m.reference_forward(x)
    r.square().sum().backward()
    assert y.shape == (4, 10) and float(y.detach().abs().max()) > 0.1
    assert float((y - r).detach().abs().max()) < 1e-9
    for n, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, n
        assert float((got[n] - p.grad).abs().max() / (p.grad.abs().max() + 1e-300)) < 1e-9, n
    if train and sd_prob > 0:
        # some block dropped some sample, and a second step draws other masks
        seeds = m._last_seeds
        keeps = torch.stack([K.drop_path_keep(4, b.sd_prob, s) for b, s in zip(m.blocks(), seeds)
                             if b.sd_prob > 0])
        assert not bool(keeps.all()) and bool(keeps.any())
        m(x)
        keeps2 = torch.stack([K.drop_path_keep(4, b.sd_prob, s)
                              for b, s in zip(m.blocks(), m._last_seeds) if b.sd_prob > 0])
        assert not torch.equal(keeps, keeps2)


def test_input_errors_raise():
    m = create_model("convnext_atto", num_classes=10)
    with pytest.raises(ValueError, match="expected"):
        m(torch.randn(2, 1, 32, 32))
    with pytest.raises(ValueError, match="multiples of 4"):
        m(torch.randn(2, 3, 34, 32))
    with pytest.raises(ValueError, match="multiples of 4"):
        m(torch.randn(2, 3, 32, 28))
    with pytest.raises(ValueError, match="no backward"):
        MF.patchify(torch.randn(1, 3, 8, 8, requires_grad=True), 4, torch.float32)


# ------------------------------------------------------------------------------ drop_path_keep
def test_drop_path_keep_depends_on_seed_and_sample_only():
    a = _ref.drop_path_keep(64, 0.3, 1234)
    assert torch.equal(a, _ref.drop_path_keep(64, 0.3, 1234))
    assert torch.equal(a[:16], _ref.drop_path_keep(16, 0.3, 1234))  # not on the batch size
    assert not torch.equal(a, _ref.drop_path_keep(64, 0.3, 1235))
    assert bool(_ref.drop_path_keep(64, 0.0, 1234).all())
    # it is the dropout hash applied to the sample index
    assert torch.equal(a, _ref.dropout_keep(64, 0.3, 1234, "cpu"))
    # the per-row scale follows the sample, whatever the map size
    f = torch.zeros(64, 5, 8)
    s = _ref._path_scale(f, 5, 0.3, 1234).reshape(64, 5)
    assert torch.equal(s != 0, a[:, None].expand(64, 5))
    assert torch.all(s[a] == torch.tensor(1.0 / 0.7, dtype=torch.float32))


def test_drop_path_keep_rate():
    n, p = 4096, 0.3
    kept = float(_ref.drop_path_keep(n, p, 2024).float().mean())
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(kept - (1 - p)) < 5 * sigma


def test_all_dropped_seed():
    """The first seed that drops all of 5 samples at p = 0.5 (chance 1/32 per seed): the GPU test
    of the all-dropped batch uses it."""
    found = next(s for s in range(4096) if not bool(_ref.drop_path_keep(5, 0.5, s).any()))
    assert found == ALL_DROPPED_SEED


def test_fold_dev_seed_matches_dispatch():
    ctr = torch.tensor([7], dtype=torch.int32)
    assert torch.equal(K.drop_path_keep(256, 0.5, K.DevSeed(99, ctr)),
                       _ref.drop_path_keep(256, 0.5, _ref.fold_dev_seed(99, 7)))
    assert _ref.fold_dev_seed(99, 7) != _ref.fold_dev_seed(99, 8)


# ------------------------------------------------------------- the contracts against autograd
def test_dwconv7_ref_equals_autograd_fp64():
    torch.manual_seed(3)
    for (N, H, W, C) in [(2, 1, 1, 8), (2, 5, 9, 8), (1, 8, 8, 16)]:
        x = torch.randn(N, H, W, C, dtype=torch.float64, requires_grad=True)
        w = torch.randn(C, 1, 7, 7, dtype=torch.float64, requires_grad=True)
        b = torch.randn(C, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(N, H, W, C, dtype=torch.float64)
        add = torch.randn(N, H, W, C, dtype=torch.float64)
        y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=C).permute(0, 2, 3, 1)
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), dy)
        wc = w.detach().permute(0, 2, 3, 1).contiguous()  # the operand layout [C, 7, 7, 1]
        assert torch.allclose(_ref.dwconv7_fwd(x.detach(), wc, b.detach()), y, rtol=0, atol=1e-12)
        assert torch.allclose(_ref.dwconv7_dgrad(dy, wc), gx, rtol=0, atol=1e-12)
        assert torch.allclose(_ref.dwconv7_dgrad(dy, wc, add), gx + add, rtol=0, atol=1e-12)
        dw, db = _ref.dwconv7_wgrad(dy, x.detach())
        assert dw.shape == (C, 1, 7, 7)
        assert torch.allclose(dw, gw, rtol=0, atol=1e-12) and torch.allclose(db, gb, rtol=0, atol=1e-12)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_scale_residual_ref_equals_autograd_fp64(p):
    torch.manual_seed(4)
    N, hw, C, seed = 6, 7, 16, 321
    f = torch.randn(N, hw, C, dtype=torch.float64, requires_grad=True)
    res = torch.randn(N, hw, C, dtype=torch.float64, requires_grad=True)
    g = torch.randn(C, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(N, hw, C, dtype=torch.float64)
    keep = _ref.drop_path_keep(N, p, seed).double()
    scale = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)) if p > 0 else 1.0
    out = res + (f * g) * (keep * scale).reshape(N, 1, 1)
    gf, gres, gg = torch.autograd.grad(out, (f, res, g), dout)
    assert torch.allclose(_ref.scale_residual_fwd(f.detach(), res.detach(), g.detach(), hw, p, seed),
                          out, rtol=0, atol=1e-12)
    df, dg, db = _ref.scale_residual_bwd(dout, f.detach(), g.detach(), hw, p, seed)
    assert torch.allclose(df, gf, rtol=0, atol=1e-12) and torch.allclose(dg, gg, rtol=0, atol=1e-12)
    assert torch.allclose(db, gf.reshape(-1, C).sum(0), rtol=0, atol=1e-12)
    assert torch.equal(gres, dout)  # the residual's gradient is dout itself: no kernel
    if p > 0:
        assert 0 < int(keep.sum()) < N


def test_functional_ops_autograd_cpu():
    """MF.dwconv7 + MF.scale_residual with the ResidualSlot / BiasGradSlot hand-offs give autograd's
    gradients of the plain composition (fp64)."""
    torch.manual_seed(5)
    N, H, W, C, p, seed = 4, 5, 6, 8, 0.5, 77
    x = torch.randn(N, H, W, C, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, 1, 7, 7, dtype=torch.float64, requires_grad=True)
    b = torch.randn(C, dtype=torch.float64, requires_grad=True)
    lw = torch.randn(C, C, dtype=torch.float64, requires_grad=True)
    lb = torch.randn(C, dtype=torch.float64, requires_grad=True)
    g = torch.randn(C, 1, 1, dtype=torch.float64, requires_grad=True)
    x2 = x * 1.0  # a non-leaf, like a block input
    slot, sb = MF.ResidualSlot(), MF.BiasGradSlot()
    y = MF.dwconv7(x2, w, w.detach().permute(0, 2, 3, 1).contiguous(), b, res_give=slot)
    f = MF.linear(y.reshape(-1, C), lw, lw.detach(), lb, bias_slot=sb).reshape(N, H, W, C)
    out = MF.scale_residual(f, x2, g, p, seed, True, bias_slot=sb, res_give=slot)
    got = torch.autograd.grad(out.square().sum(), (x, w, b, lw, lb, g))
    keep = _ref.drop_path_keep(N, p, seed).double() * float(torch.tensor(2.0))
    yr = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=C).permute(0, 2, 3, 1)
    outr = x + (F.linear(yr, lw, lb) * g.reshape(C)) * keep.reshape(N, 1, 1, 1)
    want = torch.autograd.grad(outr.square().sum(), (x, w, b, lw, lb, g))
    assert torch.allclose(out, outr, rtol=0, atol=1e-12)
    for a, r in zip(got, want):
        assert torch.allclose(a, r, rtol=0, atol=1e-10)


# ------------------------------------------------- the GPU tests' exact integer constructions
def test_exact_constructions_are_exact_in_fp32():
    """The fp32-evaluated reference of the GPU tests' integer cases equals float64: every product
    and partial sum is an integer far below 2^24 (and every output below 256, so bf16 holds it)."""
    torch.manual_seed(6)
    N, H, W, C = 3, 9, 23, 16
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s).float()  # noqa: E731
    x, dy, add = ri(-2, 2, N, H, W, C), ri(-2, 2, N, H, W, C), ri(-2, 2, N, H, W, C)
    w, b = ri(-1, 1, C, 7, 7, 1), ri(-4, 4, C)
    y32, y64 = _ref.dwconv7_fwd(x, w, b), _ref.dwconv7_fwd(x.double(), w.double(), b.double())
    assert torch.equal(y32.double(), y64) and float(y64.abs().max()) < 256
    assert torch.equal(y32.to(torch.bfloat16).double(), y64)
    g32 = _ref.dwconv7_dgrad(dy, w, add)
    g64 = _ref.dwconv7_dgrad(dy.double(), w.double(), add.double())
    assert torch.equal(g32.double(), g64) and float(g64.abs().max()) < 256
    for a, r in zip(_ref.dwconv7_wgrad(dy, x), _ref.dwconv7_wgrad(dy.double(), x.double())):
        assert torch.equal(a.double(), r)
    # scale_residual: gamma powers of two, p = 0.5 (s_n in {0, 2}), integer dout and f
    hw, Cs = 63, 96
    f, dout = ri(-3, 3, 5, hw, Cs), ri(-3, 3, 5, hw, Cs)
    gamma = torch.pow(2.0, torch.randint(-2, 3, (Cs,)).float())
    r32 = _ref.scale_residual_bwd(dout, f, gamma, hw, 0.5, 99)
    r64 = _ref.scale_residual_bwd(dout.double(), f.double(), gamma.double(), hw, 0.5, 99)
    for a, r in zip(r32, r64):
        assert torch.equal(a.double(), r)
    assert torch.equal(r32[0].to(torch.bfloat16).double(), r64[0])  # df survives bf16


# ---------------------------------------------------------------------------------- task.py
def test_task_stochastic_depth_flag(tmp_path, monkeypatch):
    """--stochastic-depth reaches the model and the metrics; the default is the family's value;
    any other arch with the flag set is a clear error."""
    import json
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mf = tmp_path / "m.json"
    args = ["--dataset", "cifar10", "--batch_size", "8", "--train-samples", "16", "--test-samples",
            "8", "--local_training", "--model_dir", str(tmp_path / "o"), "--learning_rate", "0.01",
            "--metrics-file", str(mf), "--num_epochs", "1"]
    assert T.main(args + ["--arch", "convnext_atto", "--stochastic-depth", "0.25"]) == 0
    m = json.loads(mf.read_text())
    assert m["arch"] == "convnext_atto" and m["stochastic_depth"] == 0.25 and m["steps"] == 2
    assert T.main(args + ["--arch", "convnext_atto"]) == 0
    assert json.loads(mf.read_text())["stochastic_depth"] == 0.0  # convnext_atto's own default
    with pytest.raises(SystemExit, match="convnext_\\* models only"):
        T.main(args + ["--arch", "resnet18", "--stochastic-depth", "0.1"])
    with pytest.raises(SystemExit, match=r"\[0, 1\)"):
        T.main(args + ["--arch", "convnext_atto", "--stochastic-depth", "1.5"])
    assert T.build_parser().parse_args([]).stochastic_depth is None
