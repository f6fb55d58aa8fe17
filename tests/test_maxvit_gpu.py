"""MaxViT end to end on the GPU: maxvit_nano in bf16 against its fp32 plain-torch reference, and a
captured training step replayed against eager steps."""
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


def _nano(sd_prob=0.0, seed=0):
    """maxvit_nano with larger bias tables and classifier weights (0.02 hides errors)."""
    torch.manual_seed(seed)
    m = create_model("maxvit_nano", num_classes=10, stochastic_depth_prob=sd_prob, seed=seed)
    with torch.no_grad():
        m.classifier[5].weight.normal_(std=0.1)
        for n, p in m.named_parameters():
            if n.endswith("bias_table"):
                p.normal_(std=0.5)
    return m.cuda()


def _batch(B=2, seed=5):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(B, 3, 56, 56, device=dev, generator=g),
            torch.randint(0, 10, (B,), device=dev, generator=g))


def _step_fn(m, opt):
    def step(x, y):
        opt.zero_grad()
        loss = MF.cross_entropy(m(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


def test_maxvit_nano_gpu_matches_fp32_reference():
    """B = 2 at 56 x 56 (maps 14 and 7), test_swin_gpu.py's bound for swin_nano: logits rel_err <
    5e-2 (max |difference| over max |reference|); the loss within the same fraction."""
    m = _nano()
    r = copy.deepcopy(m)
    m.compute_dtype = torch.bfloat16
    x, y = _batch(2)
    lo, lr = m(x), r.reference_forward(x)
    assert lo.dtype == torch.bfloat16 and lo.shape == lr.shape == (2, 10)
    a, b = lo.detach().double(), lr.detach().double()
    err = float((a - b).abs().max() / b.abs().max())
    loss, rloss = MF.cross_entropy(lo, y), torch.nn.functional.cross_entropy(lr, y)
    print(f"logits rel_err {err:.3e}, loss {float(loss):.5f} vs {float(rloss):.5f}")
    assert err < 5e-2
    assert abs(float(loss) - float(rloss)) < 5e-2 * float(rloss)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_graphed_training_step_replays():
    """Three AdamW steps with stochastic depth in deterministic mode: eager and a hipGraph (one
    warm-up, two replays, each drawing its own masks) give the same losses and parameters."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import AdamW
    from mipipe.train.graph import GraphedStep, graph_safe
    with deterministic(True):
        a = _nano(0.2)
        b = copy.deepcopy(a)
        opts = [AdamW(m.parameters(), lr=1e-3, weight_decay=0.01) for m in (a, b)]
        ok, why = graph_safe(b, opts[1])
        assert ok, why
        batch = _batch(2, seed=11)
        la = [_step_fn(a, opts[0])(*batch).item() for _ in range(3)]
        gs = GraphedStep(_step_fn(b, opts[1]), batch, warmup=1, inputs=[batch])
        lb = [gs.warmup_loss.item()] + [gs.replay(0).item() for _ in range(2)]
        torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n
