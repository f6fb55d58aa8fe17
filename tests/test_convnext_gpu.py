"""ConvNeXt end to end on the GPU: bf16 kernels against the fp32 plain-torch reference (with and
without stochastic depth), flat-buffer gradients, training, hipGraph replay with fresh masks,
reproducibility, and the full-size convnext_tiny path."""
import copy
import math

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


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _atto(sd_prob=0.0, seed=0, classes=10):
    """convnext_atto with layer_scale and the head re-randomised (1e-6 and zeros hide errors)."""
    torch.manual_seed(seed)
    m = create_model("convnext_atto", num_classes=classes, stochastic_depth_prob=sd_prob, seed=seed)
    with torch.no_grad():
        for b in m.blocks():
            b.layer_scale.uniform_(0.5, 1.0)
        m.classifier[2].weight.normal_(std=0.1)
        m.classifier[2].bias.normal_(std=0.1)
    return m.cuda()


def _batch(B=8, classes=10, seed=5, size=64):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(B, 3, size, size, device=dev, generator=g)
    y = torch.randint(0, classes, (B,), device=dev, generator=g)
    return x, y


@pytest.mark.parametrize("sd_prob", [0.0, 0.5])
def test_convnext_atto_gpu_matches_fp32_reference(sd_prob):
    """bf16 kernels against reference_forward in fp32 at 64 x 64, B = 4 (maps 16, 8, 4, 2), at the
    tolerances test_vit_gpu.py takes from the BERT test: logits rel_err < 5e-2, every
    parameter-gradient cosine > 0.98.  With stochastic depth the reference applies the masks the
    kernels drew; a block whose every sample was dropped has exactly-zero gradients on both
    sides (a zero vector has no direction to compare)."""
    m = _atto(sd_prob)
    r = copy.deepcopy(m)
    m.compute_dtype = torch.bfloat16
    x, y = _batch(4)
    lo = m(x)
    r._last_seeds = m._last_seeds
    lr = r.reference_forward(x)
    assert lo.dtype == torch.bfloat16 and lo.shape == lr.shape == (4, 10)
    print(f"sd {sd_prob}: logits rel_err {rel_err(lo, lr):.3e}")
    assert rel_err(lo, lr) < 5e-2
    if sd_prob > 0:
        keeps = torch.stack([K.drop_path_keep(4, b.sd_prob, s, dev)
                             for b, s in zip(m.blocks(), m._last_seeds) if b.sd_prob > 0])
        assert not bool(keeps.all()) and bool(keeps.any())
    MF.cross_entropy(lo, y).backward()
    torch.nn.functional.cross_entropy(lr, y).backward()
    rp = dict(r.named_parameters())
    worst = []
    for n, p in m.named_parameters():
        g, gr = p.grad.flatten().float(), rp[n].grad.flatten()
        if not bool(gr.any()):
            assert sd_prob > 0 and not bool(g.any()), n
            continue
        worst.append((torch.nn.functional.cosine_similarity(g, gr, 0).item(), n))
    print("lowest cosines:", sorted(worst)[:4])
    assert len(worst) > 100
    for c, n in worst:
        assert c > 0.98, (n, c)


def test_gradients_land_in_flat_buffer_once():
    """With a flat optimizer the depthwise weight / bias, layer_scale and the second Linear's bias
    gradients are accumulated by the kernels at their flat-buffer addresses and each is reported
    ready exactly once — also in a block whose samples are all dropped or kept alike."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import SGD
    from mipipe.optim.flat import flat_space_for
    m = _atto(0.5)
    ref = copy.deepcopy(m)
    opt = SGD(m.parameters(), 0.1)
    blk = m.features[5][3]
    fs = flat_space_for(blk.layer_scale)
    assert fs is not None
    names = {id(p): n for n, p in m.named_parameters()}
    seen = {}
    fs.add_ready_listener(lambda p: seen.setdefault(names[id(p)], []).append(1))
    x, y = _batch(4)
    fs.zero_grad()
    with deterministic(True):
        MF.cross_entropy(m(x), y).backward()
        MF.cross_entropy(ref(x), y).backward()
    # in every block, whatever its mask was; and nothing is reported twice
    watched = [n for n in names.values() if n.endswith(
        ("block.0.weight", "block.0.bias", "layer_scale", "block.5.bias"))]
    assert len(watched) == 4 * 12
    for n in watched:
        assert len(seen.get(n, [])) == 1, (n, len(seen.get(n, [])))
    assert all(len(v) == 1 for v in seen.values()), {n: len(v) for n, v in seen.items() if len(v) != 1}
    mp, rp = dict(m.named_parameters()), dict(ref.named_parameters())
    assert flat_space_for(ref.features[5][3].layer_scale) is None
    for n in ("features.5.3.block.0.weight", "features.5.3.block.0.bias",
              "features.5.3.layer_scale", "features.5.3.block.5.bias",
              "features.1.0.block.0.weight", "features.1.0.layer_scale"):
        p = mp[n]
        assert p.grad.data_ptr() == fs.flat_grad.data_ptr() + 4 * fs.offset(p), n
        assert float(p.grad.abs().max()) > 0, n
    # the same masks in both models (same seed, same step), so the same gradients: the fixed-order
    # sums bit for bit, the bias (summed by another kernel without the flat space) to rounding
    for n in ("features.5.3.block.0.weight", "features.5.3.block.0.bias", "features.5.3.layer_scale",
              "features.1.0.block.0.weight", "features.1.0.layer_scale"):
        assert torch.equal(mp[n].grad.reshape(-1), rp[n].grad.reshape(-1)), n
    assert rel_err(mp["features.5.3.block.5.bias"].grad, rp["features.5.3.block.5.bias"].grad) < 1e-4
    del opt


def _step_fn(m, opt):
    def step(x, y):
        opt.zero_grad()
        loss = MF.cross_entropy(m(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


@pytest.mark.parametrize("optim", ["sgd", "adamw"])
def test_convnext_atto_training_reduces_loss(optim):
    from mipipe.optim import SGD, AdamW
    m = _atto()
    opt = SGD(m.parameters(), 0.01, momentum=0.9) if optim == "sgd" \
        else AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
    step = _step_fn(m, opt)
    x, y = _batch(8)
    losses = [step(x, y).item() for _ in range(6)]
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0], losses


def test_convnext_graphed_step_matches_eager():
    """ConvNeXt (stochastic depth on) + AdamW replayed from one captured hipGraph follows the eager
    steps, within the noise measure of test_vit_graphed_step_matches_eager: the spread of two
    eager runs (the GEMM weight-grads and column sums outside deterministic mode)."""
    from mipipe.optim import AdamW
    from mipipe.train.graph import GraphedStep, graph_safe
    a = _atto(0.2)
    b, c = copy.deepcopy(a), copy.deepcopy(a)
    init = {n: p.detach().clone() for n, p in a.named_parameters()}
    opts = [AdamW(m.parameters(), lr=1e-3, weight_decay=0.01) for m in (a, b, c)]
    ok, why = graph_safe(b, opts[1])
    assert ok, why
    batch = _batch(8)
    la = [_step_fn(a, opts[0])(*batch).item() for _ in range(4)]
    lc = [_step_fn(c, opts[2])(*batch).item() for _ in range(4)]
    gs = GraphedStep(_step_fn(b, opts[1]), batch, warmup=1, inputs=[batch])
    lb = [gs.warmup_loss.item()] + [gs.replay(0).item() for _ in range(3)]
    torch.cuda.synchronize()
    assert opts[1].sync_step() == 4
    noise = max(abs(u - v) for u, v in zip(la, lc)) + 1e-3 * abs(la[0])
    assert max(abs(u - v) for u, v in zip(la, lb)) < 3 * noise + 1e-3, (la, lb, lc)
    bad = []
    for (n, p), (_, q), (_, r) in zip(a.named_parameters(), b.named_parameters(),
                                       c.named_parameters()):
        upd = float((p - init[n]).detach().norm())
        d_pq, d_pr = float((p - q).detach().norm()), float((p - r).detach().norm())
        if not d_pq <= max(0.02 * upd, 3 * d_pr) + 1e-6:
            bad.append((n, d_pq, d_pr, upd))
    assert not bad, bad


def test_replays_draw_fresh_masks():
    """With p > 0 every replay of a captured training forward draws the masks of its own step:
    two replays differ, and each equals the eager forward of that step bit for bit."""
    from mipipe.train.graph import GraphedStep
    e = _atto(0.5)
    g = copy.deepcopy(e)
    x, y = _batch(8)

    def fwd(m):
        def f(xx, yy):
            with torch.no_grad():
                return m(xx)
        return f
    eager = [fwd(e)(x, y).clone() for _ in range(3)]
    gs = GraphedStep(fwd(g), (x, y), warmup=1, inputs=[(x, y)])
    assert torch.equal(gs.warmup_loss, eager[0])
    r1 = gs.replay(0).clone()
    r2 = gs.replay(0).clone()
    torch.cuda.synchronize()
    assert not torch.equal(r1, r2)
    assert torch.equal(r1, eager[1]) and torch.equal(r2, eager[2])
    # evaluation drops nothing and does not advance the step
    e.eval()
    step = e._step
    assert torch.equal(fwd(e)(x, y), fwd(e)(x, y)) and e._step == step


def test_convnext_deterministic_mode_bit_identical_graphed_and_eager():
    """In deterministic mode two eager runs and a hipGraph-replayed run of 4 AdamW steps (with
    stochastic depth) end with bit-identical losses and parameters."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import AdamW
    from mipipe.train.graph import GraphedStep
    with deterministic(True):
        a = _atto(0.2)
        b, c = copy.deepcopy(a), copy.deepcopy(a)
        opts = [AdamW(m.parameters(), lr=1e-3, weight_decay=0.01) for m in (a, b, c)]
        batch = _batch(8, seed=11)
        la = [_step_fn(a, opts[0])(*batch).item() for _ in range(4)]
        lc = [_step_fn(c, opts[2])(*batch).item() for _ in range(4)]
        gs = GraphedStep(_step_fn(b, opts[1]), batch, warmup=1, inputs=[batch])
        lb = [gs.warmup_loss.item()] + [gs.replay(0).item() for _ in range(3)]
        torch.cuda.synchronize()
    assert la == lc and la == lb, (la, lb, lc)
    for (n, p), (_, q), (_, r) in zip(a.named_parameters(), b.named_parameters(),
                                       c.named_parameters()):
        assert torch.equal(p, r), n  # eager vs eager
        assert torch.equal(p, q), n  # eager vs graph replay


def test_convnext_tiny_full_size_forward_backward():
    """The real 56 / 28 / 14 / 7 maps at widths 96 .. 768: one forward and backward at B = 2."""
    torch.manual_seed(0)
    m = create_model("convnext_tiny")
    with torch.no_grad():
        m.classifier[2].weight.normal_(std=0.02)
        for b in m.blocks():
            b.layer_scale.fill_(0.1)
    m = m.cuda()
    x = torch.randn(2, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (2,), device=dev)
    out = m(x)
    assert out.shape == (2, 1000) and out.dtype == torch.bfloat16
    loss = MF.cross_entropy(out, y)
    loss.backward()
    assert math.isfinite(loss.item())
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), n
    assert m.features[0][0].weight.grad.abs().max() > 0
    assert m.features[1][0].block[0].weight.grad.abs().max() > 0


def test_gpu_input_errors():
    m = _atto()
    x, _ = _batch(2)
    m.compute_dtype = torch.float32
    with pytest.raises(ValueError, match="bf16"):
        m(x)
    m.compute_dtype = None
    with pytest.raises(ValueError, match="expected"):
        m(torch.randn(2, 4, 64, 64, device=dev))
    with pytest.raises(ValueError, match="multiples of 4"):
        m(torch.randn(2, 3, 66, 64, device=dev))
    assert m(x.to(torch.bfloat16)).shape == (2, 10)  # bf16 images are taken as they are
