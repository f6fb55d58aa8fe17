"""Swin V2 end to end on the GPU: swin_v2_nano in bf16 against its fp32 plain-torch reference, the
flat gradient buffer (logit scales accumulated by the attention backward), and graph replay /
reproducibility in deterministic mode."""
import copy

import pytest
import torch

from mipipe.models import create_model
from mipipe.ops import functional as MF
from mipipe.ops._native import native_available
from test_swin_gpu import _step_fn, rel_err

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    torch.manual_seed(1234)
    yield


def _nano(sd_prob=0.0, seed=0, classes=10):
    """swin_v2_nano with a larger head and position MLP (0.02 weights hide errors)."""
    torch.manual_seed(seed)
    m = create_model("swin_v2_nano", num_classes=classes, stochastic_depth_prob=sd_prob, seed=seed)
    with torch.no_grad():
        m.head.weight.normal_(std=0.1)
        for n, p in m.named_parameters():
            if "cpb_mlp" in n and p.dim() == 2:
                p.normal_(std=0.3)
    return m.cuda()


def _batch(B=4, classes=10, seed=5):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(B, 3, 128, 128, device=dev, generator=g),
            torch.randint(0, classes, (B,), device=dev, generator=g))


@pytest.mark.parametrize("sd_prob", [0.0, 0.5])
def test_swin_v2_nano_gpu_matches_fp32_reference(sd_prob):
    """B = 4 at 128 x 128 (maps 32, 16, 8: shifted and single-window stages), the bounds of
    test_swin_gpu.py: logits rel_err < 5e-2, every parameter-gradient cosine > 0.98."""
    m = _nano(sd_prob)
    r = copy.deepcopy(m)
    m.compute_dtype = torch.bfloat16
    x, y = _batch(4)
    lo = m(x)
    r._last_seeds = m._last_seeds
    lr = r.reference_forward(x)
    assert lo.dtype == torch.bfloat16 and lo.shape == lr.shape == (4, 10)
    print(f"sd {sd_prob}: logits rel_err {rel_err(lo, lr):.3e}")
    assert rel_err(lo, lr) < 5e-2
    MF.cross_entropy(lo, y).backward()
    torch.nn.functional.cross_entropy(lr, y).backward()
    rp = dict(r.named_parameters())
    worst = []
    for n, p in m.named_parameters():
        g, gr = p.grad.flatten().float(), rp[n].grad.flatten()
        if not bool(gr.any()):  # a branch whose every sample was dropped: zero on both sides
            assert sd_prob > 0 and not bool(g.any()), n
            continue
        if n.endswith("qkv.bias"):  # the K third is held at zero: exactly no gradient
            C = g.numel() // 3
            assert not bool(g[C:2 * C].any()), n
        worst.append((torch.nn.functional.cosine_similarity(g, gr, 0).item(), n))
    print("lowest cosines:", sorted(worst)[:4])
    assert len(worst) > 70  # of 105 parameters: few branches are all-dropped
    for c, n in worst:
        assert c > 0.98, (n, c)


def test_gradients_land_in_flat_buffer():
    """Every gradient is at its flat-buffer address and non-zero; the logit scales are accumulated
    there by the attention backward itself, which reports them ready once."""
    from mipipe.optim import SGD
    from mipipe.optim.flat import flat_space_for
    m = _nano()
    opt = SGD(m.parameters(), 0.1)
    fs = flat_space_for(m.head.weight)
    assert fs is not None
    names = {id(p): n for n, p in m.named_parameters()}
    seen = {}
    fs.add_ready_listener(lambda p: seen.setdefault(names[id(p)], []).append(1))
    x, y = _batch(4)
    fs.zero_grad()
    MF.cross_entropy(m(x), y).backward()
    for n, p in m.named_parameters():
        assert float(p.grad.abs().max()) > 0, n
        assert p.grad.data_ptr() == fs.flat_grad.data_ptr() + 4 * fs.offset(p), n
        times = len(seen.get(n, []))  # autograd's own accumulation does not call the listener
        assert times == 1 if n.endswith("logit_scale") else times <= 1, (n, times)


def test_deterministic_mode_bit_identical_graphed_and_eager():
    """Two eager runs and a hipGraph-replayed run of 3 AdamW steps with stochastic depth (every
    replay draws its own masks) end with bit-identical losses and parameters."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import AdamW
    from mipipe.train.graph import GraphedStep, graph_safe
    with deterministic(True):
        a = _nano(0.2)
        b, c = copy.deepcopy(a), copy.deepcopy(a)
        opts = [AdamW(m.parameters(), lr=1e-3, weight_decay=0.01) for m in (a, b, c)]
        ok, why = graph_safe(b, opts[1])
        assert ok, why
        batch = _batch(4, seed=11)
        la = [_step_fn(a, opts[0])(*batch).item() for _ in range(3)]
        lc = [_step_fn(c, opts[2])(*batch).item() for _ in range(3)]
        gs = GraphedStep(_step_fn(b, opts[1]), batch, warmup=1, inputs=[batch])
        lb = [gs.warmup_loss.item()] + [gs.replay(0).item() for _ in range(2)]
        torch.cuda.synchronize()
    assert la == lc and la == lb, (la, lb, lc)
    for (n, p), (_, q), (_, r) in zip(a.named_parameters(), b.named_parameters(),
                                       c.named_parameters()):
        assert torch.equal(p, r), n  # eager vs eager
        assert torch.equal(p, q), n  # eager vs graph replay
