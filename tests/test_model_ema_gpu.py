"""Weight EMA kernels (csrc/kernels/ema.hip) and mipipe.optim.ModelEMA on the MI355X: bits against
the fp32 reference, call gating, the in-place swap, module buffers through the device table,
hipGraph replay and evaluation of the averaged model.
Run on an MI355X:  python -m pytest tests -m gpu
"""
import copy

import numpy as np
import pytest
import torch

from mipipe.ops import _ref
from mipipe.ops._native import native_available
from mipipe.optim import SGD, ModelEMA

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    yield


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def np_weight(decay, u, warmup):
    w_min = np.float32(1.0 - decay)
    return max(w_min, np.float32(9) / np.float32(10 + u)) if warmup else w_min


class Bag(torch.nn.Module):
    """Parameters of 1, 63, 64, 65 and 8192 + 64 elements and one with reserved pad rows: two
    blocks of the flat kernels (a whole tile and a partial one) and every kind of padding."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (1, 63, 64, 65, 8192 + 64)])
        self.emb = torch.nn.Parameter(torch.randn(3, 16, generator=g))
        self.emb._mipipe_pad_rows = 8


def _bag(shadow="auto"):
    m = Bag().cuda()
    m.emb._mipipe_pad_rows = 8  # .cuda() keeps the Parameter object, the tag with it
    opt = SGD(m.parameters(), lr=0.1, shadow_dtype=shadow)
    return m, opt


def _rewrite(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g))


def _padding_is_zero(space, buf):
    for a, b, p in space.ranges():
        if bool(buf[a + p.numel():b].any()):
            return False
    return True


@pytest.mark.parametrize("decay", [0.9, 0.99998])
@pytest.mark.parametrize("warmup", [True, False])
def test_update_bits(decay, warmup):
    model, opt = _bag()
    space = opt.space
    assert space.numel % 64 == 0 and space.numel > 8192  # more than one block
    ema = ModelEMA(model, decay=decay, every=1, warmup=warmup)
    want = space.flat.detach().cpu().clone()
    for u in range(12):
        _rewrite(model, 100 + u)
        ema.update()
        w = ema.last_weight().detach().cpu()
        assert np.float32(w.item()).view(np.uint32) == np.float32(
            np_weight(decay, u, warmup)).view(np.uint32), (u, float(w))
        _ref.ema_update(want, space.flat.detach().cpu(), w)
        assert same_bits(ema.ema, want), u
        assert _padding_is_zero(space, ema.ema) and _padding_is_zero(space, space.flat)
    assert ema.num_updates() == 12
    assert not same_bits(ema.ema, space.flat)


def test_gating_every_3():
    model, opt = _bag()
    ema = ModelEMA(model, decay=0.9, every=3, warmup=True)
    changed, weights = [], []
    for call in range(1, 8):
        _rewrite(model, call)
        before, wb = ema.ema.clone(), ema.last_weight().clone()
        ema.update()
        changed.append(not same_bits(before, ema.ema))
        weights.append(not same_bits(wb, ema.last_weight()))
    assert changed == [False, False, True, False, False, True, False]
    assert weights == changed  # 0 -> 9/10 at call 3, -> 9/11 at call 6
    assert float(ema.last_weight()) == float(np.float32(9) / np.float32(11))
    assert ema.num_calls() == 7 and ema.num_updates() == 2


@pytest.mark.parametrize("shadow", ["auto", None])
def test_swap(shadow):
    model, opt = _bag(shadow)
    space = opt.space
    assert (space.shadow is not None) == (shadow == "auto")
    ema = ModelEMA(model, decay=0.9)
    _rewrite(model, 7)
    space.refresh_shadow()
    flat0, ema0 = space.flat.clone(), ema.ema.clone()
    sh0 = space.shadow.clone() if space.shadow is not None else None
    assert not same_bits(flat0, ema0)
    ptrs = (space.flat.data_ptr(), ema.ema.data_ptr())
    with ema.swapped():
        assert same_bits(space.flat, ema0) and same_bits(ema.ema, flat0)
        if sh0 is not None:
            assert torch.equal(space.shadow.view(torch.int16),
                               space.flat.to(torch.bfloat16).view(torch.int16))
        with pytest.raises(RuntimeError, match="already active"):
            with ema.swapped():
                pass
    assert same_bits(space.flat, flat0) and same_bits(ema.ema, ema0)
    if sh0 is not None:
        assert torch.equal(space.shadow.view(torch.int16), sh0.view(torch.int16))
    assert ptrs == (space.flat.data_ptr(), ema.ema.data_ptr())
    assert _padding_is_zero(space, space.flat) and _padding_is_zero(space, ema.ema)


class Buffers(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.w = torch.nn.Parameter(torch.randn(64, generator=g))
        self.base = torch.randn(8, generator=g)  # not a buffer: b5 is a view one element into it
        self.register_buffer("c58", torch.randn(58, generator=g))
        self.register_buffer("big", torch.randn(2500, generator=g))  # three table rows
        self.register_buffer("count", torch.arange(3, dtype=torch.int64))

    def attach(self):
        self.base = self.base.cuda()
        self.register_buffer("b5", self.base[1:6])
        return self


FLOAT_BUFS = ("c58", "big", "b5")


def _rewrite_buffers(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in FLOAT_BUFS:
            b = model._buffers[k]
            b.copy_(torch.randn(b.shape, generator=g))


def test_buffers_update_swap_and_rehoming():
    model = Buffers().cuda().attach()
    opt = SGD(model.parameters(), lr=0.1)
    assert model.b5.data_ptr() % 16 == 4 and model.b5.data_ptr() == model.base.data_ptr() + 4
    ema = ModelEMA(model, decay=0.9, every=1, warmup=True)
    want = {k: model._buffers[k].detach().cpu().clone() for k in FLOAT_BUFS}

    def step(seed):
        _rewrite_buffers(model, seed)
        ema.update()
        w = ema.last_weight().detach().cpu()
        for k in FLOAT_BUFS:
            _ref.ema_update(want[k], model._buffers[k].detach().cpu(), w)
        got = ema.module_state_dict()
        for k in FLOAT_BUFS:
            assert same_bits(got[k], want[k]), (seed, k)
        assert torch.equal(got["count"].cpu(), torch.arange(3)) and got["count"].dtype == torch.int64

    for s in range(3):
        step(s)
    base_edges = (float(model.base[0]), float(model.base[6]), float(model.base[7]))

    # swap: live <-> average for the float buffers, the int64 buffer untouched, then restored
    live = {k: model._buffers[k].clone() for k in FLOAT_BUFS}
    with ema.swapped():
        for k in FLOAT_BUFS:
            assert same_bits(model._buffers[k], want[k]), k
        assert torch.equal(model.count.cpu(), torch.arange(3))
    for k in FLOAT_BUFS:
        assert same_bits(model._buffers[k], live[k]), k
        assert same_bits(ema.module_state_dict()[k], want[k]), k
    assert base_edges == (float(model.base[0]), float(model.base[6]), float(model.base[7]))

    # re-home the buffers into one fresh flat tensor per dtype, as DDP's _flatten_buffers does
    old = {k: model._buffers[k] for k in FLOAT_BUFS}
    old_vals = {k: v.clone() for k, v in old.items()}
    by_dtype = {}
    for name, b in model._buffers.items():
        by_dtype.setdefault(b.dtype, []).append((name, b))
    for lst in by_dtype.values():
        flat = torch.cat([b.detach().reshape(-1) for _, b in lst])
        off = 0
        for name, b in lst:
            model._buffers[name] = flat[off:off + b.numel()].view_as(b)
            off += b.numel()
    assert all(model._buffers[k].data_ptr() != old[k].data_ptr() for k in FLOAT_BUFS)
    for s in range(3, 5):  # the next eager update() follows the new addresses
        step(s)
    for k in FLOAT_BUFS:  # and nothing wrote to the old storage
        assert same_bits(old[k], old_vals[k]), k
    with ema.swapped():
        for k in FLOAT_BUFS:
            assert same_bits(model._buffers[k], want[k]), k
    assert ema.num_updates() == 5


def _resnet_pair():
    from mipipe.models import create_model
    torch.manual_seed(0)
    a = create_model("resnet18", num_classes=10).cuda()
    models = [a, copy.deepcopy(a)]
    opts = [SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4) for m in models]
    emas = [ModelEMA(m, decay=0.99, every=2, warmup=True) for m in models]
    x = torch.randn(8, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (8,), device="cuda")
    return models, opts, emas, x, y


def _step_fn(m, o, e):
    from mipipe.ops.functional import cross_entropy

    def step(xx, yy):
        o.zero_grad()
        loss = cross_entropy(m(xx), yy)
        loss.backward()
        o.step()
        e.update()
        return loss
    return step


def _assert_same_state(emas, models):
    sa, sb = emas[0].module_state_dict(), emas[1].module_state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert same_bits(sa[k], sb[k]) if sa[k].is_floating_point() else torch.equal(sa[k], sb[k]), k
    for (n, p), (_, q) in zip(models[0].state_dict().items(), models[1].state_dict().items()):
        assert torch.equal(p, q), n


def test_graphed_resnet18_sgd_ema_equals_eager():
    from mipipe.ops.determinism import deterministic
    from mipipe.train.graph import GraphedStep, graph_safe
    with deterministic(True):
        models, opts, emas, x, y = _resnet_pair()
        ok, why = graph_safe(models[1], opts[1])
        assert ok, why
        eager = _step_fn(models[0], opts[0], emas[0])
        for _ in range(12):
            eager(x, y)
        gs = GraphedStep(_step_fn(models[1], opts[1], emas[1]), (x, y), warmup=1, inputs=[(x, y)])
        for _ in range(11):
            gs.replay(0)
        torch.cuda.synchronize()
        assert emas[0].num_updates() == 6 and emas[1].num_updates() == 6
        assert same_bits(emas[0].last_weight(), emas[1].last_weight())
        assert float(emas[1].last_weight()) == float(np.float32(9) / np.float32(15))
        assert same_bits(emas[0].ema, emas[1].ema) and same_bits(emas[0].ema_buffers,
                                                                 emas[1].ema_buffers)
        _assert_same_state(emas, models)
        live = models[1].state_dict()
        avg = emas[1].module_state_dict()
        assert not torch.equal(avg["conv1.weight"], live["conv1.weight"])
        assert not torch.equal(avg["bn1.running_mean"], live["bn1.running_mean"])
        assert torch.isfinite(emas[1].ema).all()


def test_swapped_evaluation_and_training_after():
    from mipipe.models import create_model
    from mipipe.ops import inference
    from mipipe.ops.determinism import deterministic
    with deterministic(True):
        models, opts, emas, x, y = _resnet_pair()
        steps = [_step_fn(m, o, e) for m, o, e in zip(models, opts, emas)]
        for _ in range(4):
            for s in steps:
                s(x, y)
        # a second model holding the averaged weights, with its own flat space and shadow
        ref = create_model("resnet18", num_classes=10).cuda()
        SGD(ref.parameters(), lr=0.05)
        ref.load_state_dict(emas[0].state_dict()["model"])
        ref.eval()
        models[0].eval()
        for fused in (False, True):
            with torch.no_grad(), inference.fused_eval(fused):
                want = ref(x)
                live = models[0](x)
                with emas[0].swapped():
                    got = models[0](x)
                again = models[0](x)
            assert got.shape == (8, 10) and torch.equal(got, want), fused
            assert not torch.equal(live, want)
            assert torch.equal(again, live)
        models[0].train()
        # model 0 swapped twice, model 1 never did: training goes on bit-identically
        for _ in range(2):
            for s in steps:
                s(x, y)
        torch.cuda.synchronize()
        assert emas[0].num_updates() == 3
        _assert_same_state(emas, models)
