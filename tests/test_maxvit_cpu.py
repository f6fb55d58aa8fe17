"""MaxViT on the CPU: registry, parameter count, torchvision's state_dict keys, the float64 model
against reference_forward, and _ref.partition_attention against an independent einsum."""
import pytest
import torch

from mipipe.models import create_model, model_names
from mipipe.ops import _ref


def test_registered_and_parameter_count():
    assert {"maxvit_t", "maxvit_nano"} <= set(model_names())
    with torch.device("meta"):
        m = create_model("maxvit_t")
    assert sum(p.numel() for p in m.parameters()) == 30919624  # torchvision's published figure
    assert [round(layer.sd_prob, 6) for layer in m.layers()] == [round(0.02 * i, 6)
                                                                 for i in range(11)]
    with pytest.raises(ValueError, match="multiple of 224"):
        create_model("maxvit_t")._check_input(torch.zeros(1, 3, 192, 192))


def _layer_keys(prefix, first):
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    wb = ("weight", "bias")
    keys = [f"MBconv.proj.1.{k}" for k in wb] if first else []
    keys += [f"MBconv.layers.pre_norm.{k}" for k in bn]
    for c in ("conv_a", "conv_b"):
        keys += [f"MBconv.layers.{c}.0.weight"] + [f"MBconv.layers.{c}.1.{k}" for k in bn]
    keys += [f"MBconv.layers.{m}.{k}" for m in ("squeeze_excitation.fc1", "squeeze_excitation.fc2",
                                                "conv_c") for k in wb]
    for a in ("window_attention", "grid_attention"):
        keys += [f"{a}.attn_layer.1.relative_position_bias_table",
                 f"{a}.attn_layer.1.relative_position_index"]
        keys += [f"{a}.{m}.{k}" for m in ("attn_layer.0", "attn_layer.1.to_qkv",
                                          "attn_layer.1.merge", "mlp_layer.0", "mlp_layer.1",
                                          "mlp_layer.3") for k in wb]
    return {f"{prefix}.layers.{k}" for k in keys}


def test_state_dict_keys():
    sd = create_model("maxvit_nano", num_classes=10).state_dict()
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    want = {"stem.0.0.weight", "stem.1.0.weight", "stem.1.0.bias", "classifier.2.weight",
            "classifier.2.bias", "classifier.3.weight", "classifier.3.bias", "classifier.5.weight"}
    want |= {f"stem.0.1.{k}" for k in bn}
    for b, j in ((0, 0), (1, 0), (1, 1)):
        want |= _layer_keys(f"blocks.{b}.layers.{j}", j == 0)
    assert set(sd) == want
    assert tuple(sd["blocks.1.layers.0.layers.MBconv.layers.conv_b.0.weight"].shape) == (256, 1, 3, 3)
    assert tuple(sd["blocks.1.layers.1.layers.grid_attention.attn_layer.1."
                    "relative_position_bias_table"].shape) == (169, 2)
    assert tuple(sd["blocks.0.layers.0.layers.MBconv.layers.squeeze_excitation.fc1.weight"]
                 .shape) == (8, 128, 1, 1)


@pytest.mark.parametrize("sd_prob", [0.0, 0.5])
def test_forward_matches_reference_fp64(sd_prob):
    torch.manual_seed(11)
    m = create_model("maxvit_nano", num_classes=10, stochastic_depth_prob=sd_prob,
                     compute_dtype=torch.float64, seed=5).double().train()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias_table"):
                p.normal_(std=0.5)
    x = torch.randn(4, 3, 56, 56, dtype=torch.float64)
    y = m(x)
    y.square().sum().backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    r = m.reference_forward(x)
    r.square().sum().backward()
    assert y.shape == (4, 10) and float(y.detach().abs().max()) > 0
    assert float((y - r).detach().abs().max() / r.detach().abs().max()) < 1e-9
    scale = max(float(p.grad.abs().max()) for p in m.parameters())
    for n, p in m.named_parameters():
        assert float((got[n] - p.grad).abs().max()) < 1e-9 * scale, n


def test_ref_grid_partition_against_einsum():
    """Grid mode at 14 x 21 (py = 2, px = 3) with plain strided slices: window (a, b) is
    map[a::2, b::3]."""
    B, Hs, Ws, H, D = 2, 14, 21, 2, 32
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * Hs * Ws, 3 * H * D, generator=g, dtype=torch.float64)
    table = torch.randn(169, H, generator=g, dtype=torch.float64)
    o = _ref.partition_attention(qkv, table, B, Hs, Ws, H, "grid", 0.125)
    x = qkv.reshape(B, Hs, Ws, 3, H, D)
    want = torch.empty(B, Hs, Ws, H, D, dtype=torch.float64)
    n = torch.arange(49)
    rel = (n[:, None] // 7 - n[None, :] // 7 + 6) * 13 + (n[:, None] % 7 - n[None, :] % 7 + 6)
    for a in range(2):
        for b in range(3):
            q, k, v = (x[:, a::2, b::3, i].reshape(B, 49, H, D) for i in range(3))
            s = torch.einsum("bihd,bjhd->bhij", q, k) * 0.125 + table[rel].permute(2, 0, 1)
            want[:, a::2, b::3] = torch.einsum("bhij,bjhd->bihd", s.softmax(-1),
                                               v).reshape(B, 7, 7, H, D)
    assert float((o - want.reshape(o.shape)).abs().max()) < 1e-12
