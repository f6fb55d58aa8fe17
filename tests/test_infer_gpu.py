"""Fused evaluation on the MI355X: the inference conv epilogue (csrc/kernels/conv_infer.hip) on
every tile config, operand path and split-K plan, bn_fold_affine, and whole models evaluated
with the switch of mipipe.ops.inference on.
Run on an MI355X:  python -m pytest tests -m gpu
"""
import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops import kernels as K
from mipipe.ops._native import native, native_available
from mipipe.ops.inference import fused_eval

pytestmark = pytest.mark.gpu

dev = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(1234)
    yield


# the project's bars for a conv output with the bias / ReLU epilogue (tests/test_kernels_gpu.py)
def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


TOL_OUT = {torch.bfloat16: 1e-2, torch.float32: 1e-4}
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])


def hi_ref(t):
    """Reference operand: float64 on the CPU for fp32 kernels (MIOpen has no float64 conv),
    fp32 on the GPU for bf16 kernels."""
    return t.detach().double().cpu() if t.dtype in (torch.float32, torch.float64) else t.float()


TILE_CASES = [
    # N, H, W, Ci, Co, k, s, p — dense, short-K dense, rows past M, strided, unaligned gather +
    # columns past N
    (4, 14, 14, 256, 512, 1, 1, 0),
    (8, 14, 14, 256, 64, 1, 1, 0),
    (4, 15, 13, 64, 192, 3, 1, 1),
    (4, 16, 16, 128, 256, 3, 2, 1),
    (2, 9, 7, 40, 72, 3, 1, 1),
]

SPLIT_CASES = [
    (16, 2, 2, 256, 256, 3, 1, 1),
    (32, 1, 1, 512, 512, 1, 1, 0),
    (3, 7, 5, 40, 72, 3, 1, 1),
]

# (scale + shift, residual, relu)
COMBOS = [(True, True, True), (True, False, True), (False, True, False), (False, False, False)]


@functools.lru_cache(maxsize=None)
def _case(case, dt, kw=None, pad=None):
    """Operands of a case and the reference of every combination, computed once and shared by
    the tile / plan parametrisations.  scale ~ N(0, 1): mixed signs, so a ReLU applied before
    the scale or before the residual shows."""
    N, H, W, Ci, Co, k, s, p = case
    kh, kw_ = (k, k) if kw is None else (1, kw)
    pad = p if pad is None else pad
    g = torch.Generator(device=dev).manual_seed(4321)
    r = lambda *sh: torch.randn(*sh, device=dev, generator=g)
    x = r(N, H, W, Ci).to(dt)
    w = (r(Co, kh, kw_, Ci) / math.sqrt(Ci * kh * kw_)).to(dt)
    scale, shift = r(Co), r(Co) * 0.5
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    Ho, Wo = (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw_) // s + 1
    res = r(N, Ho, Wo, Co).to(dt)
    # the fp32 coefficients go where hi_ref puts the operands of this dtype
    co = hi_ref if dt == torch.float32 else (lambda t: t)
    refs = []
    for aff, has_res, relu in COMBOS:
        refs.append(_ref.conv_fwd_infer(hi_ref(x), hi_ref(w), s, pad,
                                        co(scale) if aff else None, co(shift) if aff else None,
                                        hi_ref(res) if has_res else None, relu))
    return x, w, scale, shift, res, refs


def _run(x, w, s, pad, scale, shift, res, combo, cfg):
    aff, has_res, relu = combo
    ph, pw = (pad, -1) if isinstance(pad, int) else pad
    return native().conv_fwd_infer(x, w, s, ph, scale if aff else None, shift if aff else None,
                                   res if has_res else None, relu, 0, pw, cfg)


@pytest.mark.parametrize("cfg", list(range(15)))
@pytest.mark.parametrize("case", TILE_CASES)
@DTYPES
def test_conv_infer_every_tile(cfg, case, dt):
    """act(conv * scale + shift + residual) on every tile config: dense 1x1, aligned im2col and
    the unaligned gather, rows past M and columns past N.  With nothing to apply the launch
    gives the plain forward of the same tile bit for bit."""
    if dt == torch.float32 and cfg not in (0, 2, 8):
        pytest.skip("fp32 runs the 4-wave split-bf16x3 tiles")
    s, p = case[6], case[7]
    x, w, scale, shift, res, refs = _case(case, dt)
    for combo, ref in zip(COMBOS, refs):
        out = _run(x, w, s, p, scale, shift, res, combo, cfg)
        assert out.dtype == dt and out.shape == ref.shape
        e = rel_err(out, ref)
        assert e < TOL_OUT[dt], (combo, e)
    plain = native().conv_fwd(x, w, s, p, cfg=cfg)[0]
    assert torch.equal(out.view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                       plain.view(torch.int16 if dt == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("splits", [2, 3, 8])
@pytest.mark.parametrize("tile", [0, 1, 11])
@pytest.mark.parametrize("case", SPLIT_CASES)
@DTYPES
def test_conv_infer_split_plans(splits, tile, case, dt):
    """Split-K plans (tile + 16 x splits): the finish launch runs the inference epilogue on the
    slices summed in order; two runs of a plan are bit-identical."""
    if dt == torch.float32 and tile not in (0, 2, 8):
        pytest.skip("fp32 runs the 4-wave split-bf16x3 tiles")
    cfg = tile + 16 * splits
    s, p = case[6], case[7]
    x, w, scale, shift, res, refs = _case(case, dt)
    for combo, ref in zip(COMBOS, refs):
        out = _run(x, w, s, p, scale, shift, res, combo, cfg)
        e = rel_err(out, ref)
        assert e < TOL_OUT[dt], (combo, e)
        again = _run(x, w, s, p, scale, shift, res, combo, cfg)
        assert torch.equal(out, again), combo
    assert torch.equal(out, native().conv_fwd(x, w, s, p, cfg=cfg)[0])


@DTYPES
def test_conv_infer_rect(dt):
    """Inception's 1x7 conv: separate horizontal padding."""
    case = (2, 17, 17, 128, 128, 1, 1, 0)
    x, w, scale, shift, res, refs = _case(case, dt, 7, (0, 3))
    assert w.shape == (128, 1, 7, 128) and res.shape == (2, 17, 17, 128)
    for combo, ref in zip(COMBOS, refs):
        out = _run(x, w, 1, (0, 3), scale, shift, res, combo, -1)
        e = rel_err(out, ref)
        assert e < TOL_OUT[dt], (combo, e)
    aff, has_res, relu = COMBOS[0]
    assert torch.equal(K.conv_fwd_infer(x, w, 1, (0, 3), scale, shift, res, relu),
                       _run(x, w, 1, (0, 3), scale, shift, res, COMBOS[0], -1))


def test_conv_infer_checks_the_residual():
    x, w, scale, shift, res, _ = _case(TILE_CASES[4], torch.bfloat16)
    with pytest.raises(RuntimeError, match="residual"):
        native().conv_fwd_infer(x, w, 1, 1, None, None, res.float())
    with pytest.raises(RuntimeError, match="residual"):
        native().conv_fwd_infer(x, w, 1, 1, None, None, res[:, :-1].contiguous())
    strided = torch.cat([res, res], -1)[..., :res.shape[-1]]   # right shape, not contiguous
    with pytest.raises(RuntimeError, match="residual"):
        native().conv_fwd_infer(x, w, 1, 1, None, None, strided)


@pytest.mark.parametrize("C", [8, 72, 2048])
@pytest.mark.parametrize("with_bias", [False, True])
def test_bn_fold_affine(C, with_bias):
    gamma = torch.rand(C, device=dev) + 0.5
    beta = torch.randn(C, device=dev) * 0.1
    mean = torch.randn(C, device=dev)
    var = torch.rand(C, device=dev) + 0.05
    cb = torch.randn(C, device=dev) if with_bias else None
    eps = 1e-5
    scale, shift = native().bn_fold_affine(gamma, beta, mean, var, eps, cb)
    # the eval branch of functional.bn_stats_from_partials, plus the bias fold
    invstd = torch.rsqrt(var + eps)
    sr = gamma * invstd
    hr = beta - mean * sr
    if cb is not None:
        hr = hr + cb * sr
    assert scale.dtype == shift.dtype == torch.float32 and scale.shape == shift.shape == (C,)
    torch.testing.assert_close(scale, sr)
    torch.testing.assert_close(shift, hr)
    s2, h2 = K.bn_fold_affine(gamma, beta, mean, var, eps, cb)
    assert torch.equal(s2, scale) and torch.equal(h2, shift)


# ------------------------------------------------------------------------------------ models
def cos(a, b):
    """Scale-invariant cosine (tests/test_zoo_gpu.py)."""
    a, b = a.flatten().double(), b.flatten().double()
    a, b = a / (a.abs().max() + 1e-300), b / (b.abs().max() + 1e-300)
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def rel_l2(o, r):
    o, r = o.flatten().double(), r.flatten().double()
    return ((o - r).norm() / r.norm()).item()


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


MODELS = [("resnet18", 32), ("resnet50", 64), ("vgg11_bn", 64), ("mobilenet_v2", 64)]


@pytest.mark.parametrize("arch,res", MODELS)
@DTYPES
def test_models_fused_eval(arch, res, dt, monkeypatch):
    """Eval forward with the switch off and on against plain fp32 torch on the same weights:
    the unfused path meets the project's bar on these inputs, and so does the fused one."""
    from mipipe.models import create_model
    from mipipe.models.reference import RefVGG, ref_resnet
    torch.manual_seed(0)
    kw = {} if arch.startswith("resnet") else {"dropout": 0.0}
    m = create_model(arch, num_classes=10, **kw).cuda()
    m.compute_dtype = dt
    x = torch.randn(4, 3, res, res, device=dev)
    _settle_bn(m, x)
    if arch.startswith("resnet"):
        r = ref_resnet(arch, num_classes=10).cuda().eval()
        r.load_state_dict(m.state_dict())
        ref_fwd = r
    elif arch.startswith("vgg"):
        r = RefVGG(arch, num_classes=10, dropout=0.0).cuda().eval()
        r.load_state_dict(m.state_dict())
        ref_fwd = r
    else:
        ref_fwd = m.reference_forward
    calls = []
    real = K.conv_fwd_infer
    monkeypatch.setattr(K, "conv_fwd_infer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        ref = ref_fwd(x)
        plain = m(x)
        assert not calls
        with fused_eval():
            fused = m(x)
    assert calls, "the fused path was not taken"
    if dt == torch.bfloat16:
        cp, cf = cos(plain, ref), cos(fused, ref)
        msg = f"{arch} bf16: cos(unfused, ref) = {cp:.6f}, cos(fused, ref) = {cf:.6f}"
        print(msg)
        assert cp > 0.99, msg
        assert cf > 0.99, msg
    else:
        ep, ef = rel_l2(plain, ref), rel_l2(fused, ref)
        msg = f"{arch} fp32: |unfused - ref|/|ref| = {ep:.3e}, |fused - ref|/|ref| = {ef:.3e}"
        print(msg)
        assert ep < 1e-3, msg
        assert ef < 1e-3, msg


def test_fused_eval_follows_training():
    """The BN fold is recomputed every forward: the flat optimizer and bn_finalize write
    parameters and running statistics behind the tensors' version counters, so a cached
    (scale, shift) would make the second fused evaluation repeat the first."""
    from mipipe.models import create_model
    from mipipe.optim import SGD
    from mipipe.ops.functional import cross_entropy
    torch.manual_seed(0)
    m = create_model("resnet18", num_classes=10).cuda()
    m.compute_dtype = torch.bfloat16
    opt = SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=1e-4, shadow_dtype=torch.bfloat16)
    x = torch.randn(16, 3, 32, 32, device=dev)
    y = torch.randint(0, 10, (16,), device=dev)
    xe = torch.randn(8, 3, 32, 32, device=dev)

    def train(steps):
        m.train()
        for _ in range(steps):
            opt.zero_grad()
            cross_entropy(m(x), y).backward()
            opt.step()

    def evaluate():
        m.eval()
        with torch.no_grad():
            plain = m(xe).float()
            with fused_eval():
                fused = m(xe).float()
        return plain, fused

    train(2)
    u1, f1 = evaluate()
    assert cos(f1, u1) > 0.99, cos(f1, u1)
    train(2)
    u2, f2 = evaluate()
    assert cos(f2, u2) > 0.99, cos(f2, u2)
    d_now, d_stale = (f2 - u2).norm().item(), (f2 - u1).norm().item()
    moved = (u2 - u1).norm().item()
    assert moved > 10 * d_now, (moved, d_now)       # training moved the outputs ...
    assert d_now < 0.1 * d_stale, (d_now, d_stale)  # ... and the fused evaluation followed


def test_task_fused_eval_gpu(tmp_path):
    """task.py --fused-eval in fresh processes (the task sets process-wide modes): same seed,
    deterministic mode; the two evaluations may disagree on at most one of the 64 test samples
    (a near-tie argmax under bf16 rounding)."""
    env = dict(os.environ)
    env.pop("MIPIPE_FUSED_EVAL", None)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    acc = {}
    for fused in (0, 1):
        out = tmp_path / f"run{fused}"
        args = ["--arch", "resnet18", "--num_classes", "10", "--dataset", "cifar10",
                "--batch_size", "64", "--train-samples", "256", "--test-samples", "64",
                "--num_epochs", "1", "--steps", "4", "--local_training", "--model_dir", str(out),
                "--log-every", "0", "--gpu", "0", "--fused-eval", str(fused),
                "--metrics-file", str(out / "metrics.json")]
        r = subprocess.run([sys.executable, "-m", "mipipe.train.task"] + args, env=env,
                           capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        mt = json.loads((out / "metrics.json").read_text())
        assert mt["fused_eval"] is bool(fused) and mt["deterministic"] and mt["steps"] == 4, mt
        acc[fused] = mt["accuracy"]
    print(f"accuracy unfused {acc[0]}, fused {acc[1]}")
    assert abs(acc[0] - acc[1]) <= 1.0 / 64 + 1e-9, acc
