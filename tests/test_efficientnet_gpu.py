"""EfficientNet end to end on the GPU: bf16 kernels against the fp32 plain-torch reference,
flat-buffer gradients, the depthwise weight-grad's bits, a captured training step against eager
in deterministic mode, and eval mode."""
import copy

import pytest
import torch

from mipipe.models import create_model
from mipipe.ops import functional as MF
from mipipe.ops import kernels as K
from mipipe.ops._native import native_available

pytestmark = pytest.mark.gpu

dev = "cuda"


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(1234)
    yield


def cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    a, b = a / (a.abs().max() + 1e-300), b / (b.abs().max() + 1e-300)
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def small(sd_prob=0.2, seed=0):
    """width 0.5, depth 1.5 (the first stage gets a residual block), 10 classes, no dropout."""
    torch.manual_seed(seed)
    return create_model("efficientnet_b0", width_mult=0.5, depth_mult=1.5, num_classes=10,
                        dropout=0.0, stochastic_depth_prob=sd_prob, seed=seed).cuda()


def batch(B=8, size=64, classes=10, seed=5):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(B, 3, size, size, device=dev, generator=g),
            torch.randint(0, classes, (B,), device=dev, generator=g))


def step_fn(m, opt):
    def step(x, y):
        opt.zero_grad()
        loss = MF.cross_entropy(m(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


@pytest.mark.parametrize("which", ["small", "b0"])
def test_train_matches_fp32_reference(which):
    """Training forward and backward at 64 x 64, B = 8, with the same keep masks: cosine of the
    logits (test_mobilenetv3_gpu.py's 1 - cos < 0.01) and of the flat gradient (< 0.02).  The last
    stages normalise 8 x 2 x 2 values per channel, which amplifies bf16 rounding beyond that, so
    the tolerance is twice the distance of a bf16-cast reference_forward from the fp32 one on the
    same inputs and masks.  1 - cos of logits / flat gradient: kernels 0.034 / 0.17 (small),
    0.006 / 0.024 (b0); bf16 reference 0.051 / 0.20 (small), 0.007 / 0.030 (b0)."""
    m = small() if which == "small" else create_model("efficientnet_b0", num_classes=10,
                                                      dropout=0.0).cuda()
    r = copy.deepcopy(m)
    x, y = batch()
    lo = m(x)
    r._last_seeds = m._last_seeds
    lr = r.reference_forward(x)
    h = copy.deepcopy(r).bfloat16()  # the reference itself in bf16
    lh = h.reference_forward(x)
    assert lo.dtype == torch.bfloat16 and lo.shape == lr.shape == (8, 10)
    MF.cross_entropy(lo, y).backward()
    torch.nn.functional.cross_entropy(lr, y).backward()
    torch.nn.functional.cross_entropy(lh.float(), y).backward()

    def flat(model):
        return torch.cat([p.grad.flatten().float() for p in model.parameters()])
    assert torch.isfinite(flat(m)).all()
    assert 1 - cos(lo, lr) < max(0.01, 2 * (1 - cos(lh, lr)))
    assert 1 - cos(flat(m), flat(r)) < max(0.02, 2 * (1 - cos(flat(h), flat(r))))


def test_flat_gradients_present_and_depthwise_weight_grad_bit_identical(monkeypatch):
    """With a flat optimizer every parameter's gradient is its view of the flat buffer and is
    non-zero.  The depthwise weight-grad launched a second time in default mode on the operands
    of the same step reproduces the flat buffer's bits.  (Two whole steps are not compared: the
    dense convs' BatchNorm statistics upstream use float atomics in default mode, so the
    depthwise operands of two steps differ.)"""
    from mipipe.optim import SGD
    from mipipe.optim.flat import flat_space_for
    calls = []
    real = K.dwconvk_wgrad
    monkeypatch.setattr(K, "dwconvk_wgrad", lambda dy, x, k, s, dw=None: (
        calls.append((dy, x, k, s, dw)), real(dy, x, k, s, dw))[1])
    m = small(seed=3)
    opt = SGD(m.parameters(), 0.1)
    opt.zero_grad()
    MF.cross_entropy(m(batch()[0]), batch()[1]).backward()
    fs = flat_space_for(m.classifier[1].weight)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() == fs.flat_grad.data_ptr() + 4 * fs.offset(p), n
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    assert len(calls) == len(m.blocks())
    for dy, x, k, s, dw in calls:
        assert dw is not None and torch.equal(real(dy, x, k, s).reshape(-1), dw)
    del opt


def test_deterministic_mode_captured_step_and_eager_bit_identical():
    """In deterministic mode two eager runs and a hipGraph-replayed run of 3 SGD steps (stochastic
    depth on, the first stage's residual through the data-grad addend) end with bit-identical
    losses and parameters; the two replays draw different keep masks."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import SGD
    from mipipe.train.graph import GraphedStep, graph_safe
    with deterministic(True):
        a = small()
        b, c = copy.deepcopy(a), copy.deepcopy(a)
        opts = [SGD(m.parameters(), 0.01, momentum=0.9) for m in (a, b, c)]
        assert graph_safe(b, opts[1])[0]
        x, y = batch()
        la = [step_fn(a, opts[0])(x, y).item() for _ in range(3)]
        lc = [step_fn(c, opts[2])(x, y).item() for _ in range(3)]
        gs = GraphedStep(step_fn(b, opts[1]), (x, y), warmup=1, inputs=[(x, y)])
        lb, keeps = [gs.warmup_loss.item()], []
        for _ in range(2):
            lb.append(gs.replay(0).item())
            keeps.append(torch.stack([K.drop_path_keep(8, blk.sd_prob, s, dev) for blk, s in
                                      zip(b.blocks(), b._last_seeds) if blk.sd_prob > 0]))
    assert la == lc == lb and all(v == v for v in la), (la, lb, lc)
    assert not torch.equal(keeps[0], keeps[1]) and not bool(keeps[0].all())
    for (n, p), (_, q), (_, r) in zip(a.named_parameters(), b.named_parameters(),
                                       c.named_parameters()):
        assert torch.equal(p, r) and torch.equal(p, q), n


def test_eval_runs_through_running_statistics():
    m = small()
    x, y = batch()
    for _ in range(2):
        m(x)
    m.eval()
    with torch.no_grad():
        out, ref = m(x), m.reference_forward(x)
    assert torch.equal(out, m(x)) and cos(out, ref) > 0.99
