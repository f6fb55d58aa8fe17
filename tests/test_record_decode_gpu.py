"""Device-side record decode on the MI355X (csrc/kernels/records.hip).

The kernel must reproduce ``records.reference_transform`` — the NumPy definition the host
loader matches bit for bit — exactly: the fp32 output is compared as uint32 words.  The record
sets below are checked (with ``_splitmix64``) to contain every augmentation case: both flip
states, shifts of both signs, shifts of the full padding and no shift at all."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mipipe.data import records as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
MEANS = {1: R.MNIST_MEAN, 3: R.CIFAR10_MEAN}
STDS = {1: R.MNIST_STD, 3: R.CIFAR10_STD}
# (shape, pad, n, batch): odd 193-byte stride + partial last batch; no padding; odd width with a
# pad larger than half the image; a row wider than a wave; the CIFAR shape.  The first set has
# 47 records, not 37: 37 x 2 epochs contain no unshifted sample (the coverage test below).
CASES = [((3, 8, 8), 2, 47, 5), ((1, 28, 28), 0, 37, 5), ((3, 5, 7), 3, 37, 5),
         ((3, 3, 130), 1, 37, 5), ((3, 32, 32), 4, 80, 64)]
IDS = ["3x8x8-p2", "1x28x28-p0", "3x5x7-p3", "3x3x130-p1", "3x32x32-p4"]


def _native():
    from mipipe.ops._native import load_error, native, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"
    return native()


@functools.lru_cache(maxsize=None)
def _dataset(shape, n, label_bytes=1):
    """(records uint8 [n, rec_bytes], images, labels, global indices): the indices are shuffled,
    not 0..n-1, and one lies beyond 2**32."""
    rng = np.random.default_rng(sum(shape) + n)
    img = rng.integers(0, 256, size=(n, *shape), dtype=np.uint8)
    lab = rng.integers(0, 256 ** label_bytes if label_bytes < 2 else 1000, size=n).astype(np.int64)
    gidx = rng.permutation(4 * n)[:n].astype(np.int64)
    gidx[n // 2] += 1 << 40
    rec = np.empty((n, label_bytes + img[0].size), np.uint8)
    for k in range(label_bytes):
        rec[:, k] = (lab >> (8 * k)) & 0xFF
    rec[:, label_bytes:] = img.reshape(n, -1)
    return rec, img, lab, gidx


@functools.lru_cache(maxsize=None)
def _reference(shape, pad, n, train, epoch):
    """reference_transform of the whole set, computed once per case and shared (read-only)."""
    _, img, _, gidx = _dataset(shape, n)
    C = shape[0]
    ref = np.stack([R.reference_transform(img[i], int(gidx[i]), epoch, SEED, train,
                                          pad if train else 0, train, MEANS[C], STDS[C])
                    for i in range(n)])
    ref.setflags(write=False)
    return ref


def _affine(C, dev):
    m, s = np.asarray(MEANS[C], np.float32), np.asarray(STDS[C], np.float32)
    a = np.stack([np.float32(1.0) / (np.float32(255.0) * s), -m / s]).astype(np.float32)
    return torch.from_numpy(a).to(dev)


def _decode(rec, gidx, shape, pad, train, epoch, batch, label_bytes=1, dtype=torch.float32):
    """The native kernel over the set in batches of ``batch`` (the last one partial)."""
    nat = _native()
    dev = torch.device("cuda", 0)
    aff = _affine(shape[0], dev)
    xs, ys = [], []
    for b in range(0, len(rec), batch):
        r = torch.from_numpy(rec[b:b + batch]).to(dev)
        g = torch.from_numpy(gidx[b:b + batch]).to(dev)
        x, y = nat.record_decode(r, g, aff, *shape, SEED, epoch, pad if train else 0, train, train,
                                 label_bytes, dtype)
        xs.append(x)
        ys.append(y)
    return torch.cat(xs).cpu(), torch.cat(ys).cpu()


def _augmentations(gidx, epochs, pad):
    out = []
    for e in epochs:
        for gi in gidx.tolist():
            h = R._splitmix64(SEED ^ R._splitmix64(((e * 0x100000001B3) & R._MASK64) ^ gi))
            dy = int(h % (2 * pad + 1)) - pad if pad else 0
            dx = int((h >> 16) % (2 * pad + 1)) - pad if pad else 0
            out.append((dy, dx, (h >> 40) & 1))
    return out


@pytest.mark.parametrize("shape,pad,n,batch", CASES, ids=IDS)
def test_sample_set_covers_every_augmentation(shape, pad, n, batch):
    aug = _augmentations(_dataset(shape, n)[3], (0, 1), pad)
    assert {f for _, _, f in aug} == {0, 1}, "both flip states"
    if pad == 0:
        assert all(dy == 0 and dx == 0 for dy, dx, _ in aug)
        return
    dys, dxs = {a[0] for a in aug}, {a[1] for a in aug}
    assert min(dys) < 0 < max(dys) and min(dxs) < 0 < max(dxs), "shifts of both signs"
    assert dys & {-pad, pad} and dxs & {-pad, pad}, "|dy| = pad and |dx| = pad"
    assert any(dy == 0 and dx == 0 for dy, dx, _ in aug), "dy = dx = 0"


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("shape,pad,n,batch", CASES, ids=IDS)
def test_kernel_bit_equal_to_reference_transform(shape, pad, n, batch, train):
    rec, _, lab, gidx = _dataset(shape, n)
    for epoch in (0, 1):
        ref = _reference(shape, pad, n, train, epoch)
        x, y = _decode(rec, gidx, shape, pad, train, epoch, batch)
        assert x.dtype == torch.float32 and tuple(x.shape) == ref.shape
        got = x.numpy().view(np.uint32)
        bad = np.argwhere(got != ref.view(np.uint32))
        assert bad.size == 0, (epoch, len(bad), bad[:4].tolist())
        assert np.array_equal(y.numpy(), lab)


def test_kernel_empty_batch():
    nat = _native()
    dev = torch.device("cuda", 0)
    x, y = nat.record_decode(torch.empty(0, 193, dtype=torch.uint8, device=dev),
                             torch.empty(0, dtype=torch.int64, device=dev), _affine(3, dev),
                             3, 8, 8, SEED, 0, 2, True, True, 1, torch.float32)
    torch.cuda.synchronize()
    assert tuple(x.shape) == (0, 3, 8, 8) and x.dtype == torch.float32
    assert tuple(y.shape) == (0,) and y.dtype == torch.int64


def test_binding_rejects_bad_arguments():
    nat = _native()
    dev = torch.device("cuda", 0)
    rec = torch.zeros(2, 193, dtype=torch.uint8, device=dev)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    aff = _affine(3, dev)
    ok = (3, 8, 8, SEED, 0, 2, True, True, 1, torch.float32)
    nat.record_decode(rec, idx, aff, *ok)
    with pytest.raises(RuntimeError):  # stride does not match label_bytes + C*H*W
        nat.record_decode(rec, idx, aff, 3, 8, 8, SEED, 0, 2, True, True, 2, torch.float32)
    with pytest.raises(RuntimeError):
        nat.record_decode(rec, idx, aff, 3, 8, 8, SEED, 0, -1, True, True, 1, torch.float32)
    with pytest.raises(RuntimeError):
        nat.record_decode(rec.cpu(), idx, aff, *ok)
    with pytest.raises(RuntimeError):
        nat.record_decode(rec, idx.int(), aff, *ok)
    with pytest.raises(RuntimeError):
        nat.record_decode(rec, idx[:1], aff, *ok)
    with pytest.raises(RuntimeError):
        nat.record_decode(rec, idx, aff[:, :2].contiguous(), *ok)
    with pytest.raises(RuntimeError):
        nat.record_decode(rec, idx, aff, 3, 8, 8, SEED, 0, 2, True, True, 1, torch.float16)


@pytest.mark.parametrize("shape,pad,n,batch", CASES, ids=IDS)
def test_bf16_output_is_rounded_fp32(shape, pad, n, batch):
    rec, _, lab, gidx = _dataset(shape, n)
    x32, _ = _decode(rec, gidx, shape, pad, True, 1, batch)
    xbf, y = _decode(rec, gidx, shape, pad, True, 1, batch, dtype=torch.bfloat16)
    assert xbf.dtype == torch.bfloat16
    assert torch.equal(xbf.view(torch.int16), x32.to(torch.bfloat16).view(torch.int16))
    assert np.array_equal(y.numpy(), lab)


def test_two_byte_labels():
    shape, pad, n = (3, 8, 8), 2, 37
    rec, img, lab, gidx = _dataset(shape, n, 2)
    assert rec.shape[1] == 194 and lab.max() >= 256
    x, y = _decode(rec, gidx, shape, pad, True, 0, 5, label_bytes=2)
    assert np.array_equal(y.numpy(), lab)
    ref = np.stack([R.reference_transform(img[i], int(gidx[i]), 0, SEED, True, pad, True,
                                          MEANS[3], STDS[3]) for i in range(n)])
    assert np.array_equal(x.numpy().view(np.uint32), ref.view(np.uint32))


def test_loader_device_decode_equals_host(tmp_path):
    _native()
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(37, 3, 8, 8), dtype=np.uint8)
    lab = rng.integers(0, 10, size=37)
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    R.write_records(files[0], img[:20], lab[:20])
    R.write_records(files[1], img[20:], lab[20:])
    out = {}
    for decode in ("host", "device"):
        dl = R.RecordDataLoader(files, (3, 8, 8), batch_size=5, train=True, pad=2, seed=SEED,
                                workers=3, prefetch=2, device="cuda", decode=decode)
        assert dl.native
        dl.set_epoch(1)
        batches = list(dl)
        assert [len(y) for _, y in batches] == [5] * 7 + [2]
        out[decode] = (torch.cat([x for x, _ in batches]), torch.cat([y for _, y in batches]))
    (xh, yh), (xd, yd) = out["host"], out["device"]
    assert xd.is_cuda and xd.dtype == torch.float32
    assert torch.equal(xd, xh) and torch.equal(yd, yh)
    assert torch.equal(yd.cpu(), torch.from_numpy(lab[list(iter(dl.sampler))].astype(np.int64)))


def _run_task(tmp_path, data_dir, device_decode):
    from mipipe.launch.launcher import free_port
    out = tmp_path / f"run{device_decode}"
    env = dict(os.environ)
    for k in ("LOCAL_RANK", "GROUP_RANK"):
        env.pop(k, None)
    env.update({"WORLD_SIZE": "1", "RANK": "0", "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": str(free_port()), "HSA_ENABLE_IPC_MODE_LEGACY": "0",
                "PYTHONPATH": REPO + os.pathsep + env.get("PYTHONPATH", "")})
    args = ["--arch", "mnist_cnn", "--dataset", "mnist", "--data-dir", str(data_dir),
            "--batch_size", "64", "--num_epochs", "1", "--steps", "3", "--gpu", "0",
            "--local_training", "--model_dir", str(out), "--workers", "2",
            "--device-decode", str(device_decode), "--metrics-file", str(out / "metrics.json")]
    r = subprocess.run([sys.executable, "-m", "mipipe.train.task"] + args, env=env,
                       capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = json.loads((out / "metrics.json").read_text())
    assert m["steps"] == 3 and m["deterministic"] and m["device"].startswith("cuda"), m
    sd = torch.load(out / "resnet_distributed.pth", weights_only=True, map_location="cpu")
    return m, sd


def test_task_trains_identically_with_device_decode(tmp_path):
    data = tmp_path / "data"
    R.write_synthetic_dataset(str(data), "mnist", n_train=320, n_test=64, seed=1)
    m0, sd0 = _run_task(tmp_path, data, 0)
    m1, sd1 = _run_task(tmp_path, data, 1)
    assert m0["loss"] == m1["loss"] and m0["loss"] == m0["loss"], (m0["loss"], m1["loss"])
    assert m0["accuracy"] == m1["accuracy"]
    assert list(sd0) == list(sd1) and len(sd0) > 0
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
