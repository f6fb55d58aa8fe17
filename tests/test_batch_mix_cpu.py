"""Mixup / CutMix without a GPU: the descriptor (mipipe.data.mix), the reference contracts of
``batch_mix`` and the pair-target cross-entropy, and the trainer flags on the CPU path."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mipipe.data.mix import BatchMixer, mix_params
from mipipe.ops import _ref
from mipipe.train import task as T

SEED, H, W, STEPS = 3, 32, 48, 400
OPTS = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.8, switch_prob=0.5)


def _draw(**kw):
    o = dict(OPTS, **kw)
    return [mix_params(SEED, 0, 1, s, H, W, **o) for s in range(STEPS)]


def test_mix_params_is_a_pure_function():
    a, b = _draw(), _draw()
    assert all(p.dtype == np.float32 and p.shape == (8,) for p in a)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    other_rank = [mix_params(SEED, 1, 1, s, H, W, **OPTS) for s in range(STEPS)]
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, other_rank))
    assert len({p.tobytes() for p in a}) > STEPS // 2  # differs across steps


def test_mix_params_semantics_and_coverage():
    ps = _draw()
    modes = {int(p[1]) for p in ps}
    assert modes == {0, 1, 2}  # a skipped step (prob < 1), mixup and cutmix
    clipped = {"top": False, "bottom": False, "left": False, "right": False}
    empty = False
    for p in ps:
        lam, mode = p[0], int(p[1])
        assert 0.0 <= lam <= 1.0 and p[6] == 0 and p[7] == 0
        if mode == 0:
            assert lam == 1.0 and not p[2:6].any()
        elif mode == 1:
            assert not p[2:6].any()
        else:
            y0, y1, x0, x1 = (int(v) for v in p[2:6])
            assert p[2:6].tolist() == [y0, y1, x0, x1]  # integers, exact in fp32
            assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
            area = (y1 - y0) * (x1 - x0)
            assert lam == np.float32(1.0 - area / float(H * W))
            if area == 0:
                empty = True
                assert lam == 1.0
            else:
                clipped["top"] |= y0 == 0
                clipped["bottom"] |= y1 == H
                clipped["left"] |= x0 == 0
                clipped["right"] |= x1 == W
    assert all(clipped.values()), clipped
    assert empty


def test_mix_params_off_and_single_mode():
    for s in range(50):
        p = mix_params(SEED, 0, 0, s, H, W)
        assert p.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
        assert int(mix_params(SEED, 0, 0, s, H, W, mixup_alpha=0.4)[1]) == 1
        assert int(mix_params(SEED, 0, 0, s, H, W, cutmix_alpha=1.0)[1]) == 2
        assert int(mix_params(SEED, 0, 0, s, H, W, mixup_alpha=0.4, cutmix_alpha=1.0,
                              switch_prob=0.0)[1]) == 1
        assert int(mix_params(SEED, 0, 0, s, H, W, mixup_alpha=0.4, cutmix_alpha=1.0,
                              prob=0.0)[1]) == 0


def test_cutmix_box_follows_the_formula():
    # an unclipped box is 2 * (cut_h // 2) by 2 * (cut_w // 2) with cut_h = int(H r) and
    # cut_w = int(W r) of one ratio r = sqrt(1 - lambda): both extents are even and some r gives both
    seen = 0
    for p in _draw(prob=1.0, mixup_alpha=0.0):
        assert int(p[1]) == 2
        y0, y1, x0, x1 = (int(v) for v in p[2:6])
        if 0 < y0 and y1 < H and 0 < x0 and x1 < W:
            bh, bw = y1 - y0, x1 - x0
            assert bh % 2 == 0 and bw % 2 == 0
            assert max(bh / H, bw / W) < min((bh + 2) / H, (bw + 2) / W)
            seen += 1
    assert seen > 10


def test_batch_mixer_cpu():
    m = BatchMixer(SEED, 0, "cpu", **OPTS)
    assert m.enabled and m.mix.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    d = m.descriptor(1, 7, H, W)
    assert d is m.mix and d.dtype == torch.float32 and d.shape == (8,)
    assert d.numpy().tobytes() == mix_params(SEED, 0, 1, 7, H, W, **OPTS).tobytes()
    assert m.last_mode == int(d[1]) and m.last_lambda == float(d[0])
    d2 = m.descriptor(1, 8, H, W)
    assert d2 is d  # one device tensor, rewritten
    assert not BatchMixer(SEED, 0, "cpu").enabled


def _loop_mix(x, mix):
    B, C, Hh, Ww = x.shape
    lam, mode = np.float32(mix[0]), int(mix[1])
    y0, y1, x0, x1 = (int(v) for v in mix[2:6])
    xn = x.numpy()
    out = xn.copy()
    om = np.float32(1) - lam
    for i in range(B):
        j = B - 1 - i
        if i == j:
            continue  # its own partner: keeps its bits
        for c in range(C):
            for y in range(Hh):
                for xx in range(Ww):
                    if mode == 1:
                        out[i, c, y, xx] = np.float32(lam * xn[i, c, y, xx]) + \
                            np.float32(om * xn[j, c, y, xx])
                    elif mode == 2 and y0 <= y < y1 and x0 <= xx < x1:
                        out[i, c, y, xx] = xn[j, c, y, xx]
    return torch.from_numpy(out)


@pytest.mark.parametrize("B", [1, 2, 5])
def test_ref_batch_mix_against_loop(B):
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 2, 5, 7, generator=g)
    descs = [[1, 0, 0, 0, 0, 0, 0, 0], [0.3, 1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0],
             [1, 1, 0, 0, 0, 0, 0, 0], [0.5, 2, 1, 4, 2, 5, 0, 0], [1, 2, 3, 3, 1, 1, 0, 0],
             [0, 2, 0, 5, 0, 7, 0, 0]]
    for d in descs:
        mix = torch.tensor(d, dtype=torch.float32)
        want = _loop_mix(x, mix.numpy())
        got = _ref.batch_mix(x, mix)
        assert got is not x and torch.equal(got.view(torch.int32), want.view(torch.int32)), d
        dst = torch.empty_like(x)
        assert _ref.batch_mix(x, mix, out=dst) is dst and torch.equal(dst, want)
        xin = x.clone()
        assert _ref.batch_mix(xin, mix, out=xin) is xin and torch.equal(xin, want)
    xb = x.bfloat16()
    mix = torch.tensor([0.3, 1, 0, 0, 0, 0, 0, 0])
    want = (xb.float() * mix[0] + xb.flip(0).float() * (1 - mix[0])).bfloat16()
    if B % 2:
        want[B // 2] = xb[B // 2]
    assert torch.equal(_ref.batch_mix(xb, mix), want)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [1.0, 0.0, 0.3])
@pytest.mark.parametrize("V,valid", [(17, -1), (24, 19)])
def test_ref_cross_entropy_mixed_vs_torch(eps, lam, V, valid):
    g = torch.Generator().manual_seed(V)
    R = 9
    Vv = valid if valid > 0 else V
    x = torch.randn(R, V, generator=g, dtype=torch.float64, requires_grad=True)
    a = torch.randint(0, Vv, (R,), generator=g)
    b = a.flip(0)
    mix = torch.tensor([lam, 1, 0, 0, 0, 0, 0, 0], dtype=torch.float32)
    lam32 = float(mix[0])
    xs = x[:, :Vv]
    want = lam32 * F.cross_entropy(xs, a, label_smoothing=eps) + \
        (1 - lam32) * F.cross_entropy(xs, b, label_smoothing=eps)
    (gw,) = torch.autograd.grad(want, x)
    loss, grad = _ref.cross_entropy_mixed_fwd_bwd(x.detach(), a, mix, eps, valid)
    assert loss.dtype == torch.float64
    assert abs(float(loss) - float(want.detach())) < 1e-6
    assert (grad - gw).abs().max().item() < 1e-6
    if Vv < V:
        assert not grad[:, Vv:].any()


def test_cross_entropy_mixed_function_on_cpu():
    from mipipe.ops.functional import cross_entropy, cross_entropy_mixed
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 11, generator=g, requires_grad=True)
    y = torch.randint(0, 11, (7,), generator=g)
    mix = torch.tensor([1.0, 0, 0, 0, 0, 0, 0, 0])
    la = cross_entropy_mixed(x, y, mix, 0.1)
    (ga,) = torch.autograd.grad(la * 0.5, x)
    lb = cross_entropy(x, y, 0.1)
    (gb,) = torch.autograd.grad(lb * 0.5, x)
    assert torch.allclose(la, lb, atol=1e-6) and torch.allclose(ga, gb, atol=1e-6)


def test_parser_defaults_are_off(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = T.build_parser().parse_args([])
    assert a.label_smoothing == 0.0 and a.mixup_alpha == 0.0 and a.cutmix_alpha == 0.0
    assert a.mix_prob == 1.0 and a.mix_switch_prob == 0.5
    crit = T.CrossEntropyLoss()
    assert crit.label_smoothing == 0.0


def test_task_main_with_mixing_on_cpu(tmp_path, monkeypatch):
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = ["--arch", "mnist_cnn", "--dataset", "mnist", "--batch_size", "32",
            "--train-samples", "128", "--test-samples", "64", "--local_training",
            "--model_dir", str(tmp_path / "out"), "--learning_rate", "0.05", "--log-every", "1",
            "--log-dir", str(tmp_path / "log"), "--num_epochs", "1",
            "--metrics-file", str(tmp_path / "m.json"),
            "--mixup-alpha", "0.2", "--cutmix-alpha", "1.0", "--label-smoothing", "0.1"]
    assert T.main(args) == 0
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["steps"] == 4 and math.isfinite(m["loss"])
    assert 0.0 <= m["mix_lambda"] <= 1.0 and m["mix_mode"] in (1, 2)
    want = mix_params(0, 0, 0, 3, 28, 28, mixup_alpha=0.2, cutmix_alpha=1.0)
    assert m["mix_lambda"] == float(want[0]) and m["mix_mode"] == int(want[1])
    steps = [json.loads(ln) for ln in (tmp_path / "log" / "rank0.jsonl").read_text().splitlines()]
    steps = [s for s in steps if s["event"] == "step"]
    assert len(steps) == 4 and all("mix_lambda" in s and "mix_mode" in s for s in steps)
