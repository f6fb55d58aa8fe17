"""The "rrc" record transform (RandomResizedCrop / centre crop + bilinear resize + flip +
Normalize) without a GPU: the NumPy definition against literal golden boxes and against
``F.interpolate``, then the native host loader, the pure-Python twin and the ``_ref`` device
contract against that definition bit for bit, then task.py and the 3-step pipeline on rrc records."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mipipe.data import records as R
from mipipe.runtime import runtime, runtime_available

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))
import rrc_common as RC  # noqa: E402

SEED = RC.SEED
SMALL = RC.CASES[:4]  # the 256 -> 224 geometry runs once, on the GPU
SMALL_IDS = RC.IDS[:4]

# (seed, epoch, index, H, W) -> (y0, x0, h, w, flip), from the prototype that defined the transform
GOLDEN = [((11, 0, 3, 20, 24), (9, 9, 7, 9, 1)),
          ((11, 1, 3, 20, 24), (4, 6, 15, 13, 1)),
          ((11, 0, 2 ** 40 + 5, 256, 256), (11, 75, 164, 154, 1)),
          ((0, 0, 0, 9, 13), (0, 2, 9, 11, 1)),
          ((11, 0, 3, 6, 300), (0, 146, 6, 8, 1)),   # the fallback
          ((11, 0, 3, 300, 6), (146, 0, 8, 6, 1)),   # the fallback
          ((11, 3, 17, 40, 40), (10, 10, 18, 22, 0))]


def _need_runtime():
    if not runtime_available():
        pytest.skip("mipipe._runtime not built")


def test_golden_boxes():
    for args, box in GOLDEN:
        assert R.reference_rrc_box(*args, True) == box, args
    assert R.reference_rrc_box(11, 0, 3, 20, 24, True, flip=False) == (9, 9, 7, 9, 0)
    # evaluation: centre square of 7/8 of the short side
    assert R.reference_rrc_box(11, 5, 3, 256, 256, False) == (16, 16, 224, 224, 0)
    assert R.reference_rrc_box(11, 5, 3, 20, 24, False) == (1, 3, 17, 17, 0)


def test_golden_boxes_native():
    _need_runtime()
    for args, box in GOLDEN:
        assert tuple(runtime().rrc_box(*args, True)) == box, args


def test_ratio_table_copies_agree():
    assert len(R.RATIO_Q16) == 64
    assert list(R.RATIO_Q16) == [round(65536 * 0.75 * (16 / 9) ** (t / 63)) for t in range(64)]
    _need_runtime()
    assert tuple(runtime().rrc_ratio_q16()) == tuple(R.RATIO_Q16)


@pytest.mark.parametrize("shape,out,n,batch", RC.CASES, ids=RC.IDS)
def test_python_box_equals_native_box(shape, out, n, batch):
    _need_runtime()
    rt = runtime()
    _, H, W = shape
    for epoch in (0, 1, 7):
        for i in range(1000):
            gi = 7 * i + 3 + ((1 << 40) if i % 97 == 0 else 0)
            for train in (True, False):
                a = R.reference_rrc_box(SEED, epoch, gi, H, W, train)
                assert a == tuple(rt.rrc_box(SEED, epoch, gi, H, W, train)), (epoch, gi, train)
                y0, x0, h, w, _ = a
                assert 0 <= y0 and 0 <= x0 and h > 0 and w > 0 and y0 + h <= H and x0 + w <= W


@pytest.mark.parametrize("shape,out,n,batch", RC.CASES, ids=RC.IDS)
def test_resampling_close_to_interpolate(shape, out, n, batch):
    """Against F.interpolate(bilinear, align_corners=False) of the same box, flipped, on 0-255
    data before Normalize (mean 0, std 1/255).  Bound 0.01: the Q16 floor of a coordinate is below
    2^-16 per axis and the slope at most 255 per axis, 2 * 255 * 2^-16 = 0.0078, plus fp32 rounding."""
    _, img, _, gidx = RC.dataset(shape, n)
    C, H, W = shape
    unit = ((0.0,) * C, (1.0 / 255.0,) * C)
    worst = 0.0
    for train in (True, False):
        for i in range(min(n, 16)):
            gi = int(gidx[i])
            got = R.reference_transform_rrc(img[i], gi, 1, SEED, train, out, train, *unit)
            y0, x0, h, w, fl = R.reference_rrc_box(SEED, 1, gi, H, W, train)
            box = torch.from_numpy(img[i][:, y0:y0 + h, x0:x0 + w].astype(np.float32))[None]
            ref = F.interpolate(box, size=out, mode="bilinear", align_corners=False)[0]
            if fl:
                ref = ref.flip(-1)
            worst = max(worst, float(np.abs(got - ref.numpy()).max()))
    print(f"max |rrc - interpolate| = {worst:.5f}")
    assert worst <= 0.01


def test_identity_box_is_exactly_the_crop():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(3, 32, 32), dtype=np.uint8)
    got = R.reference_transform_rrc(img, 5, 0, SEED, False, (28, 28), False, R.CIFAR10_MEAN,
                                    R.CIFAR10_STD)
    crop = np.zeros((3, 32, 32), np.uint8)
    crop[:, :28, :28] = img[:, 2:30, 2:30]  # the centre 28x28 through the crop transform
    ref = R.reference_transform(crop, 5, 0, SEED, False, 0, False, R.CIFAR10_MEAN,
                                R.CIFAR10_STD)[:, :28, :28]
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
    # a training box of exactly the output size: crop + flip
    for gi in range(200):
        y0, x0, h, w, fl = R.reference_rrc_box(SEED, 0, gi, 20, 24, True)
        got = R.reference_transform_rrc(img[:, :20, :24], gi, 0, SEED, True, (h, w), True,
                                        R.CIFAR10_MEAN, R.CIFAR10_STD)
        box = img[:, y0:y0 + h, x0:x0 + w]
        box = box[:, :, ::-1] if fl else box
        m = np.asarray(R.CIFAR10_MEAN, np.float32)[:, None, None]
        s = np.asarray(R.CIFAR10_STD, np.float32)[:, None, None]
        ref = (box.astype(np.float32) * (1.0 / (255.0 * s)) + (-m / s)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), gi


def _files(tmp_path, shape, n, label_bytes=1):
    _, img, lab, _ = RC.dataset(shape, n, label_bytes)
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    R.write_records(files[0], img[:n // 3], lab[:n // 3], label_bytes=label_bytes)
    R.write_records(files[1], img[n // 3:], lab[n // 3:], label_bytes=label_bytes)
    return files, img, lab


def _epochs(dl, epochs=(0, 1)):
    xs, ys, order = [], [], []
    for e in epochs:
        dl.set_epoch(e)
        order.append(list(iter(dl.sampler)))
        for x, y in dl:
            xs.append(x)
            ys.append(y)
    return torch.cat(xs), torch.cat(ys), order


@pytest.mark.parametrize("no_native", [False, True], ids=["native", "python"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("shape,out,n,batch", SMALL, ids=SMALL_IDS)
def test_loader_bit_equal_to_reference(tmp_path, monkeypatch, shape, out, n, batch, train,
                                       no_native):
    """host decode (native RecordLoader, or the pure-Python twin) and decode="device" on the CPU
    device (the _ref contract) against reference_transform_rrc: epochs 0 and 1, two files, a
    partial last batch."""
    if no_native:
        monkeypatch.setenv("MIPIPE_NO_NATIVE_RUNTIME", "1")
    else:
        _need_runtime()
    files, img, lab = _files(tmp_path, shape, n)
    C = shape[0]
    res = {}
    for decode in ("host", "device"):
        dl = R.RecordDataLoader(files, shape, batch_size=batch, train=train, seed=SEED, workers=3,
                                prefetch=2, decode=decode, transform="rrc", out_size=out,
                                mean=RC.MEANS[C], std=RC.STDS[C])
        assert dl.native == (not no_native)
        assert len(dl) == -(-n // batch)
        res[decode] = _epochs(dl)
    xh, yh, order = res["host"]
    xd, yd, _ = res["device"]
    assert xh.dtype == torch.float32 and tuple(xh.shape) == (2 * n, C, *out)
    ref = np.stack([R.reference_transform_rrc(img[i], i, e, SEED, train, out, train, RC.MEANS[C],
                                              RC.STDS[C]) for e in (0, 1) for i in order[e]])
    assert np.array_equal(xh.numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(xd.numpy().view(np.uint32), ref.view(np.uint32))
    labs = torch.from_numpy(np.concatenate([lab[order[0]], lab[order[1]]]))
    assert torch.equal(yh, labs) and torch.equal(yd, labs)
    if train:
        assert not torch.equal(xh[:n], xh[n:]), "the epoch changes the boxes"


def test_two_byte_labels_round_trip(tmp_path, monkeypatch):
    shape, out, n = (3, 20, 24), (16, 16), 48
    files, img, lab = _files(tmp_path, shape, n, label_bytes=2)
    assert lab.max() >= 256
    for decode, no_native in [("host", False), ("device", False), ("host", True), ("device", True)]:
        if no_native:
            monkeypatch.setenv("MIPIPE_NO_NATIVE_RUNTIME", "1")
        elif not runtime_available():
            continue
        dl = R.RecordDataLoader(files, shape, batch_size=7, train=False, label_bytes=2,
                                decode=decode, transform="rrc", out_size=out)
        y = torch.cat([yb for _, yb in dl])
        assert torch.equal(y, torch.from_numpy(lab.astype(np.int64))), (decode, no_native)


def test_bf16_and_argument_checks(tmp_path):
    shape, out, n = (3, 20, 24), (16, 16), 48
    files, _, _ = _files(tmp_path, shape, n)
    kw = dict(batch_size=5, train=True, seed=SEED, decode="device", transform="rrc", out_size=out)
    x32, _, _ = _epochs(R.RecordDataLoader(files, shape, **kw), (0,))
    xbf, _, _ = _epochs(R.RecordDataLoader(files, shape, out_dtype=torch.bfloat16, **kw), (0,))
    assert xbf.dtype == torch.bfloat16 and torch.equal(xbf, x32.to(torch.bfloat16))
    with pytest.raises(ValueError):
        R.RecordDataLoader(files, shape, 5, transform="resize")
    with pytest.raises(ValueError):
        R.RecordDataLoader(files, shape, 5, out_size=(16, 16))  # crop keeps the stored size
    with pytest.raises(ValueError):
        R.RecordDataLoader(files, shape, 5, transform="rrc", out_size=(0, 16))
    # default out_size: the stored size
    dl = R.RecordDataLoader(files, shape, 5, transform="rrc")
    assert tuple(next(iter(dl))[0].shape) == (5, 3, 20, 24)


def test_synthetic_dataset_is_written_in_chunks(tmp_path):
    """Chunked writing draws the same stream: a set larger than one chunk equals the images
    generated in one piece (the generator the parent commit used)."""
    shape, ncls, n = (3, 40, 40), 300, 700  # 436 records per chunk
    man = R.write_synthetic_dataset(str(tmp_path), "imagenet", n_train=n, n_test=3, seed=2,
                                    num_classes=ncls, shape=shape, label_bytes=2)
    assert man["shape"] == [3, 40, 40] and man["label_bytes"] == 2
    assert R.dataset_files(str(tmp_path), "imagenet", "train") == [man["files"]["train"]]
    img, y = R.read_records(man["files"]["train"], shape, label_bytes=2)
    base = np.random.default_rng(2).normal(0.0, 1.0, size=(ncls, 3, 10, 10))
    templates = np.kron(base, np.ones((1, 1, 4, 4)))
    r = np.random.default_rng(2 * 1000 + 1)
    y0 = r.integers(0, ncls, size=n)
    x0 = 0.8 * templates[y0] + r.normal(0.0, 1.0, size=(n, *shape))
    assert np.array_equal(y, y0)
    assert np.array_equal(img, np.clip(x0 * 40.0 + 128.0, 0, 255).astype(np.uint8))


def test_task_reads_manifest_and_trains_on_rrc_records(tmp_path, monkeypatch):
    import mipipe.train.task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    data = tmp_path / "data"
    man = R.write_synthetic_dataset(str(data), "imagenet", n_train=96, n_test=32, seed=1,
                                    num_classes=300, shape=(3, 40, 40), label_bytes=2)
    (data / "manifest.json").write_text(json.dumps(man))
    out = tmp_path / "out"
    args = ["--arch", "mnist_cnn", "--dataset", "imagenet", "--image-size", "32",
            "--data-dir", str(data), "--batch_size", "32", "--num_epochs", "1",
            "--local_training", "--model_dir", str(out), "--learning_rate", "0.05",
            "--log-every", "0", "--workers", "2", "--metrics-file", str(tmp_path / "m.json")]
    assert T.main(args) == 0
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["steps"] == 3 and m["loss"] == m["loss"]
    sd = torch.load(out / "resnet_distributed.pth", weights_only=True)
    assert sd["fc2.weight"].shape[0] == 300       # class count from the manifest
    assert sd["conv1.weight"].shape[1] >= 3
    a = T.build_parser().parse_args([])
    assert a.record_transform is None
    # an explicit crop keeps the stored 40x40 (and still reads the 2-byte labels)
    assert T.main(args + ["--record-transform", "crop", "--steps", "1"]) == 0


def test_three_step_pipeline_on_rrc_records(tmp_path, gcs_root):
    import three_step_pipeline as P
    serving = tmp_path / "serving"
    rc = P.main(["--gpus", "0", "--arch", "mnist_cnn", "--dataset", "imagenet",
                 "--record-size", "40", "--image-size", "32", "--num-classes", "300",
                 "--epochs", "1", "--batch-size", "32", "--n-train", "64", "--n-test", "32",
                 "--lr", "0.05", "--baseline-accuracy", "0", "--serving-dir", str(serving),
                 "--spec", str(tmp_path / "spec.json")])
    assert rc == 0  # PIPELINE_STATE_SUCCEEDED
    man = [os.path.join(r, "manifest.json") for r, _, fs in os.walk(gcs_root)
           if "manifest.json" in fs]
    assert len(man) == 1
    m = json.load(open(man[0]))
    assert m["shape"] == [3, 40, 40] and m["label_bytes"] == 2 and m["num_classes"] == 300
    assert m["mean"] == list(R.IMAGENET_MEAN)
    assert any("model.pth" in fs for _, _, fs in os.walk(serving))
