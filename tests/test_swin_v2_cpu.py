"""Swin V2 on the CPU: the cosine window-attention contract against an independent float64
definition (torch.roll, explicit partition, F.normalize, autograd), float64 parity of ``forward``
with ``reference_forward``, parameter counts and torchvision's state-dict layout."""
import math

import pytest
import torch
import torch.nn.functional as F

from mipipe.models import create_model
from mipipe.ops import _ref

COUNTS = {"swin_v2_t": 28_351_570, "swin_v2_s": 49_737_442, "swin_v2_b": 87_930_848}


def plain_window_attention_v2(qkv, bias, logit_scale, B, Hs, Ws, heads, shift):
    """torchvision's V2 shifted_window_attention after the QKV projection, written out."""
    sy, sx = shift
    x = torch.roll(qkv.reshape(B, Hs, Ws, -1), (-sy, -sx), (1, 2))
    nW = (Hs // 8) * (Ws // 8)
    x = x.view(B, Hs // 8, 8, Ws // 8, 8, 3, heads, 32).permute(5, 0, 1, 3, 6, 2, 4, 7)
    q, k, v = x.reshape(3, B, nW, heads, 64, 32)
    a = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-1, -2)
    a = a * torch.clamp(logit_scale, max=math.log(100.0)).exp().view(heads, 1, 1)
    c = torch.stack(torch.meshgrid(torch.arange(8), torch.arange(8), indexing="ij")).flatten(1)
    d = c[:, :, None] - c[:, None, :] + 7
    a = a + bias[d[0] * 15 + d[1]].permute(2, 0, 1)
    img = torch.zeros(Hs, Ws)
    for i, hs in enumerate(((0, -8), (-8, -sy), (-sy, None))):
        for j, ws in enumerate(((0, -8), (-8, -sx), (-sx, None))):
            img[hs[0]:hs[1], ws[0]:ws[1]] = 3 * i + j
    img = img.view(Hs // 8, 8, Ws // 8, 8).permute(0, 2, 1, 3).reshape(nW, 64)
    a = a + ((img[:, None, :] != img[:, :, None]) * -100.0)[None, :, None]
    o = (F.softmax(a, -1) @ v).view(B, Hs // 8, Ws // 8, heads, 8, 8, 32)
    o = o.permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hs, Ws, heads * 32)
    return torch.roll(o, (sy, sx), (1, 2)).reshape(B * Hs * Ws, heads * 32)


@pytest.mark.parametrize("B,Hs,Ws,heads,shift", [
    (1, 8, 8, 1, (0, 0)), (2, 16, 16, 3, (4, 4)), (1, 16, 24, 2, (4, 4)), (1, 8, 16, 2, (0, 4))])
def test_ref_window_attention_v2_equals_autograd_fp64(B, Hs, Ws, heads, shift):
    g = torch.Generator().manual_seed(Hs * Ws + heads)
    f64 = dict(generator=g, dtype=torch.float64)
    qkv = torch.randn(B * Hs * Ws, 3 * heads * 32, **f64).requires_grad_()
    bias = (16 * torch.rand(225, heads, **f64)).requires_grad_()
    ls = torch.tensor([math.log(10.0), math.log(200.0), -1.0][:heads], dtype=torch.float64,
                      requires_grad=True)
    do = torch.randn(B * Hs * Ws, heads * 32, **f64)
    want = plain_window_attention_v2(qkv, bias, ls, B, Hs, Ws, heads, shift)
    grads = torch.autograd.grad(want, (qkv, bias, ls), do)
    args = (qkv.detach(), bias.detach(), ls.detach(), B, Hs, Ws, heads, shift)
    got = _ref.window_attention_v2(*args, do)
    assert torch.equal(got[0], _ref.window_attention_v2(*args))
    for a, r in zip(got, (want.detach(),) + grads):
        assert float((a - r).abs().max()) < 1e-10 and float(r.abs().max()) > 0.1
    if heads > 1:
        assert float(got[3][1]) == 0.0  # ln 200 is clamped


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("sd_prob", [0.0, 0.5])
def test_forward_matches_reference_fp64(sd_prob, train):
    torch.manual_seed(11)
    m = create_model("swin_v2_nano", num_classes=10, stochastic_depth_prob=sd_prob,
                     compute_dtype=torch.float64, seed=5).double()
    with torch.no_grad():  # 1-d parameters, logit scales and the k bias at their init hide errors
        for n, p in m.named_parameters():
            if p.dim() == 1 or n.endswith("logit_scale"):
                p.add_(torch.randn_like(p) * 0.2)
    m.train(train)
    x = torch.randn(4, 3, 128, 128, dtype=torch.float64)
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
        if n.endswith("qkv.bias"):  # the (non-zero) k bias is not used: no gradient
            C = p.numel() // 3
            assert not got[n][C:2 * C].any() and got[n][:C].any() and got[n][2 * C:].any()


@pytest.mark.parametrize("arch", list(COUNTS))
def test_parameter_counts(arch):
    with torch.device("meta"):
        m = create_model(arch)
    total = 48 * m.dims[0] + 3 * m.dims[0]  # stem conv + bias + LayerNorm
    for i, (n, c, h) in enumerate(zip(m.depths, m.dims, m.num_heads)):
        # qkv, proj, two LayerNorms, the MLP, logit_scale, cpb_mlp (2 -> 512 with bias, 512 -> h)
        total += n * (3 * c * c + 3 * c + c * c + c + 4 * c + 8 * c * c + 5 * c + h
                      + 3 * 512 + 512 * h)
        if i < 3:
            total += 8 * c * c + 4 * c  # reduction (no bias) + LayerNorm(2c)
    total += 2 * m.dims[-1] + 1000 * m.dims[-1] + 1000
    assert sum(p.numel() for p in m.parameters()) == total == COUNTS[arch]
    assert m.blocks()[0].sd_prob == 0.0 and m.blocks()[-1].sd_prob == pytest.approx(
        {"swin_v2_t": 0.2, "swin_v2_s": 0.3, "swin_v2_b": 0.5}[arch])


def test_state_dict_keys_and_errors():
    m = create_model("swin_v2_nano", num_classes=10)
    sd = m.state_dict()
    blk = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
           "attn.proj.bias", "attn.logit_scale", "attn.cpb_mlp.0.weight", "attn.cpb_mlp.0.bias",
           "attn.cpb_mlp.2.weight", "attn.relative_coords_table", "attn.relative_position_index",
           "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")
    want = {f"features.{s}.{n}.{k}" for s in (1, 3, 5) for n in (0, 1) for k in blk}
    want |= {f"features.{s}.{k}" for s in (2, 4)
             for k in ("reduction.weight", "norm.weight", "norm.bias")}
    want |= {f"{p}.{k}" for p in ("features.0.0", "features.0.2", "norm", "head")
             for k in ("weight", "bias")}
    assert set(sd) == want
    shapes = {"3.1.attn.logit_scale": (2, 1, 1), "3.1.attn.cpb_mlp.0.bias": (512,),
              "3.1.attn.cpb_mlp.2.weight": (2, 512), "2.norm.weight": (64,),
              "2.reduction.weight": (64, 128), "1.0.attn.relative_coords_table": (1, 15, 15, 2),
              "1.0.attn.relative_position_index": (4096,)}
    for k, shp in shapes.items():
        assert tuple(sd["features." + k].shape) == shp, k
    t = sd["features.1.0.attn.relative_coords_table"][0]
    v = math.log2(9) / 3
    assert not t[7, 7].any() and t[14, 0].tolist() == pytest.approx([v, -v])
    assert float(sd["features.1.0.attn.logit_scale"][0]) == pytest.approx(math.log(10.0))
    with pytest.raises(ValueError, match="multiples of 128"):
        m(torch.randn(1, 3, 112, 128))
