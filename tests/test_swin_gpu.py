"""Swin end to end on the GPU: swin_nano in bf16 against its fp32 plain-torch reference, the flat
gradient buffer (bias tables included), and graph replay / reproducibility in deterministic mode."""
import copy

import pytest
import torch

from mipipe.models import create_model
from mipipe.ops import functional as MF
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
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _nano(sd_prob=0.0, seed=0, classes=10):
    """swin_nano with larger bias tables and 1-d parameters (0.02 tables hide errors)."""
    torch.manual_seed(seed)
    m = create_model("swin_nano", num_classes=classes, stochastic_depth_prob=sd_prob, seed=seed)
    with torch.no_grad():
        m.head.weight.normal_(std=0.1)
        for n, p in m.named_parameters():
            if n.endswith("bias_table"):
                p.normal_(std=0.5)
    return m.cuda()


def _batch(B=4, classes=10, seed=5):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(B, 3, 112, 112, device=dev, generator=g),
            torch.randint(0, classes, (B,), device=dev, generator=g))


def _step_fn(m, opt):
    def step(x, y):
        opt.zero_grad()
        loss = MF.cross_entropy(m(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


@pytest.mark.parametrize("sd_prob", [0.0, 0.5])
def test_swin_nano_gpu_matches_fp32_reference(sd_prob):
    """B = 4 at 112 x 112 (maps 28, 14, 7: shifted and single-window stages), the bounds of
    test_vit_gpu.py: logits rel_err < 5e-2, every parameter-gradient cosine > 0.98."""
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
        if not bool(gr.any()):
            # a branch whose every sample was dropped: exactly zero on both sides (a zero vector
            # has no direction to compare), as in test_convnext_gpu.py
            assert sd_prob > 0 and not bool(g.any()), n
            continue
        if n.endswith("qkv.bias"):
            # the KEY bias has an exactly-zero gradient (softmax is shift-invariant per query):
            # its bf16 value is rounding noise without a direction — compare Q and V
            C = g.numel() // 3
            g, gr = torch.cat([g[:C], g[2 * C:]]), torch.cat([gr[:C], gr[2 * C:]])
        worst.append((torch.nn.functional.cosine_similarity(g, gr, 0).item(), n))
    print("lowest cosines:", sorted(worst)[:4])
    assert len(worst) > 60  # of 87 parameters: few branches are all-dropped
    for c, n in worst:
        assert c > 0.98, (n, c)


def test_gradients_land_in_flat_buffer():
    """With a flat optimizer every gradient is at its flat-buffer address, non-zero, and reported
    ready once; the bias tables are accumulated there by the attention backward itself."""
    from mipipe.optim import SGD
    from mipipe.optim.flat import flat_space_for
    m = _nano()
    opt = SGD(m.parameters(), 0.1)
    tables = {n: p for n, p in m.named_parameters() if n.endswith("bias_table")}
    fs = flat_space_for(next(iter(tables.values())))
    assert fs is not None and len(tables) == 6
    names = {id(p): n for n, p in m.named_parameters()}
    seen = {}
    fs.add_ready_listener(lambda p: seen.setdefault(names[id(p)], []).append(1))
    x, y = _batch(4)
    fs.zero_grad()
    MF.cross_entropy(m(x), y).backward()
    for n, p in m.named_parameters():
        assert float(p.grad.abs().max()) > 0, n
    for n, p in tables.items():
        assert p.grad.data_ptr() == fs.flat_grad.data_ptr() + 4 * fs.offset(p), n
        assert len(seen.get(n, [])) == 1, (n, seen.get(n))
    del opt


def test_deterministic_mode_bit_identical_graphed_and_eager():
    """In deterministic mode two eager runs and a hipGraph-replayed run of 3 AdamW steps (with
    stochastic depth: every replay draws its own masks) end with bit-identical losses and
    parameters."""
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


def test_gpu_input_errors():
    m = _nano()
    x, _ = _batch(2)
    m.compute_dtype = torch.float32
    with pytest.raises(ValueError, match="bf16"):
        m(x)
    m.compute_dtype = None
    with pytest.raises(ValueError, match="multiples of 112"):
        m(torch.randn(2, 3, 96, 96, device=dev))
