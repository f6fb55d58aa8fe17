"""Device-side record decode, the parts that need no GPU: the native loader's raw mode, the
``decode="device"`` option on the CPU device (pure-PyTorch contract ``ops._ref.record_decode``)
against ``decode="host"``, multi-byte labels and the synthetic writer's new arguments."""
import numpy as np
import pytest
import torch

from mipipe.data import records as R
from mipipe.runtime import runtime, runtime_available

native = pytest.mark.skipif(not runtime_available(), reason="mipipe._runtime not built")


def _write(tmp_path, n=37, shape=(3, 8, 8), classes=10, label_bytes=1, seed=0):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, *shape), dtype=np.uint8)
    lab = rng.integers(0, classes, size=n)
    f1, f2 = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    R.write_records(f1, img[:20], lab[:20], label_bytes=label_bytes)
    R.write_records(f2, img[20:], lab[20:], label_bytes=label_bytes)
    return [f1, f2], img, lab


@native
def test_raw_mode_yields_source_records_and_indices(tmp_path):
    files, img, lab = _write(tmp_path)
    rec_bytes = 1 + 3 * 8 * 8
    src = np.concatenate([np.fromfile(f, dtype=np.uint8).reshape(-1, rec_bytes) for f in files])
    assert src.shape == (37, rec_bytes)
    cfg = runtime().LoaderConfig()
    cfg.files = files
    cfg.C, cfg.H, cfg.W = 3, 8, 8
    cfg.batch, cfg.workers, cfg.prefetch = 5, 3, 2
    cfg.mean, cfg.std = list(R.CIFAR10_MEAN), list(R.CIFAR10_STD)
    cfg.raw = True
    ld = runtime().RecordLoader(cfg)
    assert len(ld) == 37 and ld.record_bytes() == rec_bytes
    sampler = R.DistributedSampler(37, num_replicas=2, rank=1, shuffle=True, seed=3)
    rec = np.zeros((5, rec_bytes), np.uint8)
    gi = np.zeros(5, np.int64)
    # the rank's 19 shuffled samples for two epochs (last batch 4), then all 37 (last batch 2)
    for epoch in (0, 1, 2):
        sampler.set_epoch(epoch)
        idx = list(iter(sampler)) if epoch < 2 else list(range(37))
        ld.start_epoch(idx, epoch)
        assert ld.batches_per_epoch() == -(-len(idx) // 5)
        got_rec, got_idx, sizes = [], [], []
        while True:
            n = ld.next_raw_into(rec.ctypes.data, gi.ctypes.data)
            if n == 0:
                break
            sizes.append(n)
            got_rec.append(rec[:n].copy())
            got_idx.append(gi[:n].copy())
        assert sizes == [5] * (len(idx) // 5) + ([len(idx) % 5] if len(idx) % 5 else [])
        assert sizes[-1] == (4 if epoch < 2 else 2)  # the partial last batch
        assert np.concatenate(got_idx).tolist() == idx
        assert np.array_equal(np.concatenate(got_rec), src[idx])
    with pytest.raises(Exception):
        ld.next_into(rec.ctypes.data, gi.ctypes.data)  # the float path is off in raw mode


def _epochs(dl, epochs=(0, 1)):
    xs, ys = [], []
    for e in epochs:
        dl.set_epoch(e)
        for x, y in dl:
            xs.append(x)
            ys.append(y)
    return torch.cat(xs), torch.cat(ys)


@pytest.mark.parametrize("no_native", [False, True])
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("shape,pad", [((3, 8, 8), 2), ((3, 5, 7), 3)])
def test_device_decode_on_cpu_equals_host(tmp_path, monkeypatch, shape, pad, train, no_native):
    if no_native:
        monkeypatch.setenv("MIPIPE_NO_NATIVE_RUNTIME", "1")
    elif not runtime_available():
        pytest.skip("mipipe._runtime not built")
    files, img, lab = _write(tmp_path, shape=shape)
    out = {}
    for decode in ("host", "device"):
        sampler = R.DistributedSampler(37, num_replicas=2, rank=1, shuffle=True, seed=3)
        dl = R.RecordDataLoader(files, shape, batch_size=5, sampler=sampler, train=train,
                                pad=pad, seed=11, workers=3, prefetch=2, decode=decode)
        assert dl.native == (not no_native)
        out[decode] = _epochs(dl)
    (xh, yh), (xd, yd) = out["host"], out["device"]
    assert xd.dtype == torch.float32 and xd.shape == xh.shape and xh.shape[0] == 2 * 19
    assert torch.equal(xd, xh)
    assert torch.equal(yd, yh)


def test_device_decode_bf16_on_cpu(tmp_path):
    files, img, lab = _write(tmp_path)
    kw = dict(batch_size=5, train=True, pad=2, seed=11, decode="device")
    x32, _ = _epochs(R.RecordDataLoader(files, (3, 8, 8), **kw), (0,))
    xbf, _ = _epochs(R.RecordDataLoader(files, (3, 8, 8), out_dtype=torch.bfloat16, **kw), (0,))
    assert xbf.dtype == torch.bfloat16 and torch.equal(xbf, x32.to(torch.bfloat16))


def test_two_byte_labels_round_trip(tmp_path, monkeypatch):
    files, img, lab = _write(tmp_path, classes=1000, label_bytes=2, seed=4)
    lab[:3] = (999, 256, 255)
    R.write_records(files[0], img[:20], lab[:20], label_bytes=2)
    assert lab.max() == 999
    x, y = R.read_records(files[0], (3, 8, 8), label_bytes=2)
    assert np.array_equal(x, img[:20]) and np.array_equal(y, lab[:20])
    raw = np.fromfile(files[0], dtype=np.uint8).reshape(20, 2 + 192)
    assert raw[0, 0] == 999 & 0xFF and raw[0, 1] == 999 >> 8  # little-endian
    with pytest.raises(ValueError):
        R.write_records(str(tmp_path / "bad.bin"), img[:2], [3, 256], label_bytes=1)
    modes = [("host", False), ("device", False), ("host", True), ("device", True)]
    for decode, no_native in modes:
        if no_native:
            monkeypatch.setenv("MIPIPE_NO_NATIVE_RUNTIME", "1")
        elif not runtime_available():
            continue
        dl = R.RecordDataLoader(files, (3, 8, 8), batch_size=8, train=False, label_bytes=2,
                                decode=decode)
        y = torch.cat([yb for _, yb in dl])
        assert torch.equal(y, torch.from_numpy(lab.astype(np.int64))), (decode, no_native)


def test_synthetic_dataset_shape_and_label_bytes(tmp_path):
    man = R.write_synthetic_dataset(str(tmp_path), "wide", n_train=600, n_test=40,
                                    shape=(3, 16, 16), num_classes=300, label_bytes=2)
    assert man["shape"] == [3, 16, 16] and man["label_bytes"] == 2 and man["num_classes"] == 300
    x, y = R.read_records(man["files"]["train"], (3, 16, 16), label_bytes=2)
    assert x.shape == (600, 3, 16, 16) and x.dtype == np.uint8
    assert 256 <= y.max() < 300 and y.min() >= 0
    xt, yt = R.read_records(man["files"]["test"], man["shape"], label_bytes=man["label_bytes"])
    assert xt.shape == (40, 3, 16, 16) and yt.max() < 300
    dl = R.RecordDataLoader([man["files"]["test"]], (3, 16, 16), 16, train=False, label_bytes=2,
                            decode="device")
    assert torch.equal(torch.cat([yb for _, yb in dl]), torch.from_numpy(yt))
