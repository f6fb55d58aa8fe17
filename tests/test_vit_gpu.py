"""Vision Transformer end to end on the GPU: bf16 kernels against the fp32 plain-torch reference,
flat-buffer gradients, training, reproducibility, and the full-size vit_b_16 path."""
import copy
import math

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
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


def _tiny(patch=16, seed=0, classes=10):
    """vit_tiny with a randomised head and class token (zero-initialised ones hide errors)."""
    torch.manual_seed(seed)
    m = create_model("vit_tiny", num_classes=classes, patch_size=patch)
    with torch.no_grad():
        m.heads.head.weight.normal_(std=0.1)
        m.heads.head.bias.normal_(std=0.1)
        m.class_token.normal_(std=0.1)
    return m.cuda()


def _batch(B=8, classes=10, seed=5):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn(B, 3, 64, 64, device=dev, generator=g)
    y = torch.randint(0, classes, (B,), device=dev, generator=g)
    return x, y


@pytest.mark.parametrize("patch", [16, 32])
def test_vit_tiny_gpu_matches_fp32_reference(patch):
    """bf16 kernels against reference_forward in fp32, B = 4, S = 17 (patch 16) and S = 5 (patch
    32), at the tolerances of test_bert_tiny_gpu_matches_fp32_reference: logits rel_err < 5e-2,
    every parameter-gradient cosine > 0.98 (class_token, pos_embedding and conv_proj included)."""
    m = _tiny(patch)
    r = copy.deepcopy(m)
    m.compute_dtype = torch.bfloat16
    x, y = _batch(4)
    lo = m(x)
    lr = r.reference_forward(x)
    assert lo.dtype == torch.bfloat16 and lo.shape == lr.shape
    print(f"patch {patch}: logits rel_err {rel_err(lo, lr):.3e}")
    assert rel_err(lo, lr) < 5e-2
    MF.cross_entropy(lo, y).backward()
    torch.nn.functional.cross_entropy(lr, y).backward()
    rp = dict(r.named_parameters())
    worst = []
    for n, p in m.named_parameters():
        g, gr = p.grad.flatten().float(), rp[n].grad.flatten()
        if n.endswith("in_proj_bias"):
            # the KEY bias has an exactly-zero gradient (softmax is shift-invariant per query):
            # its bf16 value is rounding noise without a direction — compare Q and V
            D = g.numel() // 3
            g, gr = torch.cat([g[:D], g[2 * D:]]), torch.cat([gr[:D], gr[2 * D:]])
        c = torch.nn.functional.cosine_similarity(g, gr, 0).item()
        worst.append((c, n))
    print("lowest cosines:", sorted(worst)[:4])
    for c, n in worst:
        assert c > 0.98, (n, c)


def test_class_token_and_pos_embedding_gradients_land_in_flat_buffer():
    """With a flat optimizer attached the token-assembly backward accumulates the class_token and
    pos_embedding gradients straight into the flat gradient buffer and reports them ready, as the
    LayerNorm kernels do for their parameters."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import SGD
    from mipipe.optim.flat import flat_space_for
    m = _tiny()
    ref = copy.deepcopy(m)
    opt = SGD(m.parameters(), 0.1)
    fs = flat_space_for(m.class_token)
    assert fs is not None and flat_space_for(m.encoder.pos_embedding) is fs
    watched = {id(m.class_token): "class_token", id(m.encoder.pos_embedding): "pos_embedding",
               id(m.encoder.ln.weight): "encoder.ln.weight"}
    seen = {}
    fs.add_ready_listener(
        lambda p: seen.setdefault(watched[id(p)], []).append(fs.grad_view(p).clone())
        if id(p) in watched else None)
    x, y = _batch(4)
    fs.zero_grad()
    with deterministic(True):  # no float atomics: the two backward passes below see the same bits
        MF.cross_entropy(m(x), y).backward()
        MF.cross_entropy(ref(x), y).backward()
    for name in watched.values():
        assert len(seen.get(name, [])) == 1, (name, seen.keys())
    for p, name in ((m.class_token, "class_token"), (m.encoder.pos_embedding, "pos_embedding")):
        assert p.grad.data_ptr() == fs.flat_grad.data_ptr() + 4 * fs.offset(p)
        assert torch.equal(seen[name][0], p.grad) and p.grad.abs().max() > 0
    # the same gradients as the autograd path of a model without a flat space: the token sums
    # bit for bit (one owner per element either way), the GEMM-produced ones to fp32 rounding
    assert flat_space_for(ref.class_token) is None
    mp, rp = dict(m.named_parameters()), dict(ref.named_parameters())
    for n in ("class_token", "encoder.pos_embedding"):
        assert torch.equal(mp[n].grad, rp[n].grad), n
    for n in ("conv_proj.weight", "conv_proj.bias"):
        assert rel_err(mp[n].grad, rp[n].grad) < 1e-4, n
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
def test_vit_tiny_training_reduces_loss(optim):
    from mipipe.optim import SGD, AdamW
    m = _tiny()
    opt = SGD(m.parameters(), 0.01, momentum=0.9) if optim == "sgd" \
        else AdamW(m.parameters(), lr=1e-3, weight_decay=0.05)
    step = _step_fn(m, opt)
    x, y = _batch(8)
    losses = [step(x, y).item() for _ in range(6)]
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0], losses


def test_vit_graphed_step_matches_eager():
    """ViT + AdamW replayed from one captured hipGraph follows the eager steps.  Outside
    deterministic mode the attention backward keeps float atomics (dQ), which AdamW amplifies for
    near-zero gradients, so — as in test_bert_graphed_step_matches_eager — parameters are
    compared by norm against the spread of two eager runs."""
    from mipipe.optim import AdamW
    from mipipe.train.graph import GraphedStep, graph_safe
    a = _tiny()
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
    assert lb[0] == la[0]  # the eager warm-up step is the eager step
    noise = max(abs(u - v) for u, v in zip(la, lc)) + 1e-3 * abs(la[0])
    assert max(abs(u - v) for u, v in zip(la, lb)) < 3 * noise + 1e-3, (la, lb, lc)
    bad = []
    for (n, p), (_, q), (_, r) in zip(a.named_parameters(), b.named_parameters(),
                                       c.named_parameters()):
        i0 = init[n]
        if n.endswith("in_proj_bias"):  # the key bias: exactly-zero gradient, pure noise
            H = p.shape[0] // 3
            keep = torch.cat([torch.arange(0, H), torch.arange(2 * H, 3 * H)]).to(p.device)
            p, q, r, i0 = p[keep], q[keep], r[keep], i0[keep]
        upd = float((p - i0).detach().norm())
        d_pq, d_pr = float((p - q).detach().norm()), float((p - r).detach().norm())
        if not d_pq <= max(0.02 * upd, 3 * d_pr) + 1e-6:
            bad.append((n, d_pq, d_pr, upd))
    assert not bad, bad


def test_vit_deterministic_mode_bit_identical_graphed_and_eager():
    """In deterministic mode two eager runs and a hipGraph-replayed run of 4 AdamW steps end with
    bit-identical losses and parameters: the token-assembly sums have one owner per element and
    the attention backward sums dQ in order."""
    from mipipe.ops.determinism import deterministic
    from mipipe.optim import AdamW
    from mipipe.train.graph import GraphedStep
    with deterministic(True):
        a = _tiny()
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


def test_vit_b_16_full_size_forward_backward():
    """The real S = 197, H = 768 path: one forward and backward at B = 2, 224 x 224."""
    torch.manual_seed(0)
    m = create_model("vit_b_16")
    with torch.no_grad():
        m.heads.head.weight.normal_(std=0.02)
    m = m.cuda()
    x = torch.randn(2, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (2,), device=dev)
    out = m(x)
    assert out.shape == (2, 1000)
    loss = MF.cross_entropy(out, y)
    loss.backward()
    assert math.isfinite(loss.item())
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert m.conv_proj.weight.grad.abs().max() > 0 and m.class_token.grad.abs().max() > 0


def test_gpu_input_errors():
    m = _tiny()
    x, _ = _batch(2)
    m.compute_dtype = torch.float32
    with pytest.raises(ValueError, match="bf16"):
        m(x)
    m.compute_dtype = None
    with pytest.raises(ValueError, match="not interpolated"):
        m(torch.randn(2, 3, 96, 96, device=dev))
    assert m(x.to(torch.bfloat16)).shape == (2, 10)  # bf16 images are taken as they are
