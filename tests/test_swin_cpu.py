"""Swin on the CPU: the window-attention contract against an independent float64 definition
(torch.roll, explicit partition, autograd), float64 parity of ``forward`` with
``reference_forward``, parameter counts and torchvision's state-dict layout."""
import pytest
import torch
import torch.nn.functional as F

from mipipe.models import create_model
from mipipe.ops import _ref

COUNTS = {"swin_t": 28_288_354, "swin_s": 49_606_258, "swin_b": 87_768_224}


def plain_window_attention(qkv, table, B, Hs, Ws, heads, shift):
    """torchvision's shifted_window_attention after the QKV projection, written out."""
    sy, sx = shift
    x = torch.roll(qkv.reshape(B, Hs, Ws, -1), (-sy, -sx), (1, 2))
    nW = (Hs // 7) * (Ws // 7)
    x = x.view(B, Hs // 7, 7, Ws // 7, 7, 3, heads, 32).permute(5, 0, 1, 3, 6, 2, 4, 7)
    q, k, v = x.reshape(3, B, nW, heads, 49, 32)
    c = torch.stack(torch.meshgrid(torch.arange(7), torch.arange(7), indexing="ij")).flatten(1)
    d = c[:, :, None] - c[:, None, :] + 6
    a = q @ k.transpose(-1, -2) / 32 ** 0.5 + table[d[0] * 13 + d[1]].permute(2, 0, 1)
    img = torch.zeros(Hs, Ws)
    count = 0
    for hs in ((0, -7), (-7, -sy), (-sy, None)):
        for ws in ((0, -7), (-7, -sx), (-sx, None)):
            img[hs[0]:hs[1], ws[0]:ws[1]] = count
            count += 1
    img = img.view(Hs // 7, 7, Ws // 7, 7).permute(0, 2, 1, 3).reshape(nW, 49)
    a = a + ((img[:, None, :] != img[:, :, None]) * -100.0)[None, :, None]
    o = (F.softmax(a, -1) @ v).view(B, Hs // 7, Ws // 7, heads, 7, 7, 32)
    o = o.permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hs, Ws, heads * 32)
    return torch.roll(o, (sy, sx), (1, 2)).reshape(B * Hs * Ws, heads * 32)


@pytest.mark.parametrize("B,Hs,Ws,heads,shift", [
    (1, 7, 7, 1, (0, 0)), (2, 14, 14, 3, (3, 3)), (1, 14, 21, 2, (3, 3)), (1, 7, 14, 2, (0, 3)),
    (1, 7, 7, 1, (3, 3))])
def test_ref_window_attention_equals_autograd_fp64(B, Hs, Ws, heads, shift):
    g = torch.Generator().manual_seed(Hs * Ws + heads)
    qkv = torch.randn(B * Hs * Ws, 3 * heads * 32, generator=g, dtype=torch.float64,
                      requires_grad=True)
    table = torch.randn(169, heads, generator=g, dtype=torch.float64, requires_grad=True)
    do = torch.randn(B * Hs * Ws, heads * 32, generator=g, dtype=torch.float64)
    want = plain_window_attention(qkv, table, B, Hs, Ws, heads, shift)
    gq, gt = torch.autograd.grad(want, (qkv, table), do)
    o, dqkv, dtable = _ref.window_attention(qkv.detach(), table.detach(), B, Hs, Ws, heads, shift,
                                            do)
    assert torch.equal(o, _ref.window_attention(qkv.detach(), table.detach(), B, Hs, Ws, heads,
                                                shift))
    for a, r in ((o, want.detach()), (dqkv, gq), (dtable, gt)):
        assert float((a - r).abs().max()) < 1e-9 and float(r.abs().max()) > 0.1


def test_ref_patch_merge_round_trip():
    x = torch.arange(2 * 4 * 6 * 8, dtype=torch.float64).reshape(2 * 4 * 6, 8)
    y = _ref.patch_merge(x, 2, 4, 6)
    v = x.reshape(2, 4, 6, 8)
    assert torch.equal(y.reshape(2, 2, 3, 32)[1, 1, 2], torch.cat([v[1, 2, 4], v[1, 3, 4],
                                                                   v[1, 2, 5], v[1, 3, 5]]))
    assert torch.equal(_ref.patch_merge_bwd(y, 2, 4, 6), x)
    with pytest.raises(ValueError, match="even"):
        _ref.patch_merge(torch.zeros(15, 8), 1, 3, 5)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("sd_prob", [0.0, 0.5])
def test_forward_matches_reference_fp64(sd_prob, train):
    torch.manual_seed(11)
    m = create_model("swin_nano", num_classes=10, stochastic_depth_prob=sd_prob,
                     compute_dtype=torch.float64, seed=5).double()
    with torch.no_grad():  # small tables and 1-d parameters at their init hide errors
        for n, p in m.named_parameters():
            if p.dim() == 1 or n.endswith("bias_table"):
                p.add_(torch.randn_like(p) * 0.2)
    m.train(train)
    x = torch.randn(4, 3, 112, 112, dtype=torch.float64)
    y = m(x)
    y.square().sum().backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    r = m.reference_forward(x)
    r.square().sum().backward()
    assert y.shape == (4, 10) and float(y.detach().abs().max()) > 0.01
    assert float((y - r).detach().abs().max()) < 1e-9
    for n, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, n
        assert float((got[n] - p.grad).abs().max() / (p.grad.abs().max() + 1e-300)) < 1e-9, n


@pytest.mark.parametrize("arch", list(COUNTS))
def test_parameter_counts(arch):
    with torch.device("meta"):
        m = create_model(arch)
    C, total = m.dims[0], 48 * m.dims[0] + 3 * m.dims[0]  # stem conv + bias + LayerNorm
    for i, (n, c, h) in enumerate(zip(m.depths, m.dims, m.num_heads)):
        # qkv, proj, two LayerNorms, the MLP, the table
        total += n * (3 * c * c + 3 * c + c * c + c + 4 * c + 8 * c * c + 5 * c + 169 * h)
        if i < 3:
            total += 8 * c * c + 8 * c  # reduction (no bias) + LayerNorm(4c)
    total += 2 * m.dims[-1] + 1000 * m.dims[-1] + 1000
    assert sum(p.numel() for p in m.parameters()) == total == COUNTS[arch]
    sd = {"swin_t": 0.2, "swin_s": 0.3, "swin_b": 0.5}[arch]
    ps = [b.sd_prob for b in m.blocks()]
    assert ps[0] == 0.0 and ps == pytest.approx([sd * i / (len(ps) - 1) for i in range(len(ps))])


def test_state_dict_keys_and_errors():
    m = create_model("swin_nano", num_classes=10)
    keys = set(m.state_dict())
    want = {"features.0.0.weight", "features.0.0.bias", "features.0.2.weight",
            "features.0.2.bias", "norm.weight", "norm.bias", "head.weight", "head.bias"}
    for s in (1, 3, 5):
        for n in (0, 1):
            want |= {f"features.{s}.{n}.{k}" for k in (
                "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias",
                "attn.proj.weight", "attn.proj.bias", "attn.relative_position_bias_table",
                "attn.relative_position_index", "norm2.weight", "norm2.bias", "mlp.0.weight",
                "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")}
    for s in (2, 4):
        want |= {f"features.{s}.reduction.weight", f"features.{s}.norm.weight",
                 f"features.{s}.norm.bias"}
    assert keys == want
    try:
        from torchvision.models import swin_t
    except Exception:
        swin_t = None
    if swin_t is not None:
        with torch.device("meta"):
            ours, tv = create_model("swin_t"), swin_t()
        a, b = ours.state_dict(), tv.state_dict()
        assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    sd = m.state_dict()
    assert tuple(sd["features.3.1.attn.relative_position_bias_table"].shape) == (169, 2)
    assert tuple(sd["features.2.reduction.weight"].shape) == (64, 128)
    assert not sd["head.bias"].any() and sd["features.1.0.mlp.0.weight"].abs().max() <= 2.0
    with pytest.raises(ValueError, match="multiples of 112"):
        m(torch.randn(1, 3, 56, 112))
    with pytest.raises(ValueError, match="head width"):
        create_model("swin_nano").__class__(48, (2,), (1,))
