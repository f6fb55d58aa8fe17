"""RegNet end to end on the GPU (the two test-size models): bf16 kernels against the fp32
plain-torch reference, the grouped-conv route, flat-buffer gradients, two identical steps and a
captured training step against eager in deterministic mode."""
import copy

import pytest
import torch

from mipipe.models import create_model
from mipipe.models._zoo import gconv3_route
from mipipe.ops import functional as MF
from mipipe.ops._native import native_available

pytestmark = pytest.mark.gpu

dev = "cuda"
NAMES = ["regnet_x_nano", "regnet_y_nano"]


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


def small(name, seed=0):
    torch.manual_seed(seed)
    return create_model(name, num_classes=10).cuda()


def batch(B=8, size=32, classes=10, seed=5):
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


@pytest.mark.parametrize("name", NAMES)
def test_train_matches_fp32_reference_on_the_gconv3_route(name):
    """Training forward and backward at 32 x 32, B = 8: test_efficientnet_gpu.py's measure, 1 - cos
    of the logits < 0.01 and of the flat gradient < 0.02, or twice the distance of a bf16-cast
    reference_forward from the fp32 one on the same inputs where that is larger.  Every f.b conv
    (group widths 8 and 24, both strides) takes the gconv3 route."""
    m = small(name)
    r = copy.deepcopy(m)
    x, y = batch()
    for blk in m.blocks():
        conv = blk.f.b[0]
        probe = torch.empty(8, 4, 4, conv.in_channels, device=dev, dtype=torch.bfloat16)
        assert gconv3_route(probe, conv) and not gconv3_route(probe.float(), conv)
    lo = m(x)
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
    print("1 - cos logits / grads:", 1 - cos(lo, lr), 1 - cos(flat(m), flat(r)),
          "bf16 reference:", 1 - cos(lh, lr), 1 - cos(flat(h), flat(r)))
    assert 1 - cos(lo, lr) < max(0.01, 2 * (1 - cos(lh, lr)))
    assert 1 - cos(flat(m), flat(r)) < max(0.02, 2 * (1 - cos(flat(h), flat(r))))


def test_flat_gradients_land_in_the_flat_buffer():
    from mipipe.optim import SGD
    from mipipe.optim.flat import flat_space_for
    m = small("regnet_y_nano", seed=3)
    opt = SGD(m.parameters(), 0.1)
    opt.zero_grad()
    MF.cross_entropy(m(batch()[0]), batch()[1]).backward()
    fs = flat_space_for(m.fc.weight)
    for n, p in m.named_parameters():
        assert p.grad.data_ptr() == fs.flat_grad.data_ptr() + 4 * fs.offset(p), n
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    del opt


@pytest.mark.parametrize("name", NAMES)
def test_deterministic_mode_captured_step_and_eager_bit_identical(name):
    """In deterministic mode two eager runs and a hipGraph-replayed run of 3 SGD steps end with
    bit-identical losses and parameters."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import SGD
    from mipipe.train.graph import GraphedStep, graph_safe
    with deterministic(True):
        a = small(name)
        b, c = copy.deepcopy(a), copy.deepcopy(a)
        opts = [SGD(m.parameters(), 0.01, momentum=0.9) for m in (a, b, c)]
        assert graph_safe(b, opts[1])[0]
        x, y = batch()
        la = [step_fn(a, opts[0])(x, y).item() for _ in range(3)]
        lc = [step_fn(c, opts[2])(x, y).item() for _ in range(3)]
        gs = GraphedStep(step_fn(b, opts[1]), (x, y), warmup=1, inputs=[(x, y)])
        lb = [gs.warmup_loss.item()] + [gs.replay(0).item() for _ in range(2)]
    assert la == lc == lb and all(v == v for v in la), (la, lb, lc)
    for (n, p), (_, q), (_, r) in zip(a.named_parameters(), b.named_parameters(),
                                       c.named_parameters()):
        assert torch.equal(p, r) and torch.equal(p, q), n


def test_eval_runs_through_running_statistics():
    m = small("regnet_y_nano")
    x, _ = batch()
    for _ in range(2):
        m(x)
    m.eval()
    with torch.no_grad():
        out, ref = m(x), m.reference_forward(x)
    assert torch.equal(out, m(x)) and cos(out, ref) > 0.99
