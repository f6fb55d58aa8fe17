"""The "rrc" record transform on the MI355X (csrc/kernels/records.hip record_decode_rrc).

The kernel must reproduce ``records.reference_transform_rrc`` — the NumPy definition the host
loader matches bit for bit (test_record_rrc_cpu.py) — exactly: fp32 outputs are compared as uint32
words.  The record sets (tests/rrc_common.py) are first checked to contain every geometry the
later tests rely on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mipipe.data import records as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rrc_common as RC  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = RC.SEED


def _native():
    from mipipe.ops._native import load_error, native, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"
    return native()


def _affine(C, dev):
    m, s = np.asarray(RC.MEANS[C], np.float32), np.asarray(RC.STDS[C], np.float32)
    a = np.stack([np.float32(1.0) / (np.float32(255.0) * s), -m / s]).astype(np.float32)
    return torch.from_numpy(a).to(dev)


def _decode(rec, gidx, shape, out, train, epoch, batch, label_bytes=1, dtype=torch.float32):
    """The native kernel over the set in batches of ``batch`` (the last one may be partial)."""
    nat = _native()
    dev = torch.device("cuda", 0)
    aff = _affine(shape[0], dev)
    xs, ys = [], []
    for b in range(0, len(rec), batch):
        r = torch.from_numpy(rec[b:b + batch].copy()).to(dev)
        g = torch.from_numpy(gidx[b:b + batch].copy()).to(dev)
        x, y = nat.record_decode_rrc(r, g, aff, *shape, *out, SEED, epoch, train, train,
                                     label_bytes, dtype)
        xs.append(x)
        ys.append(y)
    return torch.cat(xs).cpu(), torch.cat(ys).cpu()


@pytest.mark.parametrize("shape,out,n,batch", RC.CASES, ids=RC.IDS)
def test_sample_set_covers_every_geometry(shape, out, n, batch):
    bx = RC.boxes(shape, n)
    _, H, W = shape
    assert {b[4] for b in bx} == {0, 1}, "both flip states"
    assert all(0 <= b[0] and 0 <= b[1] and b[2] > 0 and b[3] > 0 and b[0] + b[2] <= H
               and b[1] + b[3] <= W for b in bx)
    if shape == (3, 6, 300):
        assert all(b[5] == -1 for b in bx), "every sample takes the fallback"
        assert all(b[2:4] == (6, 8) for b in bx)
    if shape in ((3, 20, 24), (3, 40, 40)):
        assert any(b[2] < out[0] and b[3] < out[1] for b in bx), "a box smaller than the output"
        assert any(b[2] > out[0] and b[3] > out[1] for b in bx), "a box larger than the output"
        assert any(b[0] == 0 or b[1] == 0 or b[0] + b[2] == H or b[1] + b[3] == W for b in bx), \
            "a box touching an image edge"
        assert any(b[5] >= 1 for b in bx), "an accepted attempt after a rejected one"
    assert int(RC.dataset(shape, n)[3].max()) > 1 << 32


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("shape,out,n,batch", RC.CASES, ids=RC.IDS)
def test_kernel_bit_equal_to_reference_transform_rrc(shape, out, n, batch, train):
    rec, _, lab, gidx = RC.dataset(shape, n)
    for epoch in (0, 1):
        ref = RC.reference(shape, out, n, train, epoch)
        x, y = _decode(rec, gidx, shape, out, train, epoch, batch)
        assert x.dtype == torch.float32 and tuple(x.shape) == ref.shape
        got = x.numpy().view(np.uint32)
        bad = np.argwhere(got != ref.view(np.uint32))
        assert bad.size == 0, (epoch, len(bad), bad[:4].tolist())
        assert np.array_equal(y.numpy(), lab)


@pytest.mark.parametrize("shape,out,n,batch", RC.CASES, ids=RC.IDS)
def test_bf16_output_is_rounded_fp32(shape, out, n, batch):
    rec, _, lab, gidx = RC.dataset(shape, n)
    x32, _ = _decode(rec, gidx, shape, out, True, 1, batch)
    xbf, y = _decode(rec, gidx, shape, out, True, 1, batch, dtype=torch.bfloat16)
    assert xbf.dtype == torch.bfloat16
    assert torch.equal(xbf.view(torch.int16), x32.to(torch.bfloat16).view(torch.int16))
    assert np.array_equal(y.numpy(), lab)


def test_bf16_four_wide_rows():
    """Wo % 8 == 4: the 8-byte bf16 store path, which no case above takes."""
    shape, out, n = (3, 20, 24), (6, 12), 48
    rec, img, lab, gidx = RC.dataset(shape, n)
    x32, _ = _decode(rec, gidx, shape, out, True, 0, 7)
    ref = np.stack([R.reference_transform_rrc(img[i], int(gidx[i]), 0, SEED, True, out, True,
                                              RC.MEANS[3], RC.STDS[3]) for i in range(n)])
    assert np.array_equal(x32.numpy().view(np.uint32), ref.view(np.uint32))
    xbf, _ = _decode(rec, gidx, shape, out, True, 0, 7, dtype=torch.bfloat16)
    assert torch.equal(xbf.view(torch.int16), x32.to(torch.bfloat16).view(torch.int16))


def test_two_byte_labels():
    shape, out, n = (3, 20, 24), (16, 16), 48
    rec, img, lab, gidx = RC.dataset(shape, n, 2)
    assert rec.shape[1] == 2 + 3 * 20 * 24 and lab.max() >= 256
    x, y = _decode(rec, gidx, shape, out, True, 0, 5, label_bytes=2)
    assert np.array_equal(y.numpy(), lab)
    ref = np.stack([R.reference_transform_rrc(img[i], int(gidx[i]), 0, SEED, True, out, True,
                                              RC.MEANS[3], RC.STDS[3]) for i in range(n)])
    assert np.array_equal(x.numpy().view(np.uint32), ref.view(np.uint32))


def test_kernel_empty_batch():
    nat = _native()
    dev = torch.device("cuda", 0)
    x, y = nat.record_decode_rrc(torch.empty(0, 1441, dtype=torch.uint8, device=dev),
                                 torch.empty(0, dtype=torch.int64, device=dev), _affine(3, dev),
                                 3, 20, 24, 16, 16, SEED, 0, True, True, 1, torch.float32)
    torch.cuda.synchronize()
    assert tuple(x.shape) == (0, 3, 16, 16) and x.dtype == torch.float32
    assert tuple(y.shape) == (0,) and y.dtype == torch.int64


def test_binding_rejects_bad_arguments():
    nat = _native()
    dev = torch.device("cuda", 0)
    rec = torch.zeros(2, 1441, dtype=torch.uint8, device=dev)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    aff = _affine(3, dev)
    ok = (3, 20, 24, 16, 16, SEED, 0, True, True, 1, torch.float32)
    nat.record_decode_rrc(rec, idx, aff, *ok)

    def bad(*args):
        with pytest.raises(RuntimeError):
            nat.record_decode_rrc(*args)

    bad(rec.cpu(), idx, aff, *ok)
    bad(rec, idx.cpu(), aff, *ok)
    bad(rec, idx, aff.cpu(), *ok)
    bad(rec.int(), idx, aff, *ok)
    bad(rec, idx.int(), aff, *ok)
    bad(rec, idx, aff.double(), *ok)
    bad(rec, idx[:1], aff, *ok)
    bad(rec, idx, aff[:, :2].contiguous(), *ok)
    bad(rec, idx, aff.t().contiguous(), *ok)
    bad(rec, idx, aff, 3, 20, 24, 0, 16, SEED, 0, True, True, 1, torch.float32)
    bad(rec, idx, aff, 3, 20, 24, 16, -1, SEED, 0, True, True, 1, torch.float32)
    bad(rec, idx, aff, 3, 20, 24, 16, 16, SEED, 0, True, True, 0, torch.float32)
    bad(rec, idx, aff, 3, 20, 24, 16, 16, SEED, 0, True, True, 9, torch.float32)
    bad(rec, idx, aff, 3, 20, 24, 16, 16, SEED, 0, True, True, 2, torch.float32)  # stride
    bad(rec, idx, aff, 3, 20, 24, 16, 16, SEED, 0, True, True, 1, torch.float16)
    bad(rec, idx, aff, 3, 20, 24, 16, 1 << 20, SEED, 0, True, True, 1, torch.float32)  # LDS tables


def test_loader_device_decode_equals_host(tmp_path):
    _native()
    shape, out, n = (3, 20, 24), (16, 16), 48
    _, img, lab, _ = RC.dataset(shape, n)
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    R.write_records(files[0], img[:20], lab[:20])
    R.write_records(files[1], img[20:], lab[20:])
    for train in (True, False):
        res = {}
        for decode in ("host", "device"):
            dl = R.RecordDataLoader(files, shape, batch_size=5, train=train, seed=SEED, workers=3,
                                    prefetch=2, device="cuda", decode=decode, transform="rrc",
                                    out_size=out, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
            assert dl.native
            dl.set_epoch(1)
            batches = list(dl)
            assert [len(y) for _, y in batches] == [5] * 9 + [3]
            res[decode] = (torch.cat([x for x, _ in batches]), torch.cat([y for _, y in batches]))
        (xh, yh), (xd, yd) = res["host"], res["device"]
        assert xd.is_cuda and xd.dtype == torch.float32 and tuple(xd.shape) == (n, 3, 16, 16)
        assert torch.equal(xd, xh) and torch.equal(yd, yh)
        order = list(iter(dl.sampler))
        assert torch.equal(yd.cpu(), torch.from_numpy(lab[order].astype(np.int64)))
        ref = np.stack([R.reference_transform_rrc(img[i], i, 1, SEED, train, out, train,
                                                  R.IMAGENET_MEAN, R.IMAGENET_STD) for i in order])
        assert np.array_equal(xd.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _find(node, key):
    """Every value stored under ``key`` anywhere in a JSON document."""
    if isinstance(node, dict):
        for k, v in node.items():
            if k == key:
                yield v
            yield from _find(v, key)
    elif isinstance(node, list):
        for v in node:
            yield from _find(v, key)


def test_three_step_pipeline_imagenet_shape_on_gpu(tmp_path, gcs_root):
    """preprocess (72x72 records, 1000 classes, 2-byte labels) -> train (ResNet-50 at 64x64,
    RandomResizedCrop decoded on the GPU) -> evaluate (7/8 centre crop, on the GPU) -> deploy."""
    sys.path.insert(0, os.path.join(REPO, "examples"))
    import three_step_pipeline as P
    serving = tmp_path / "serving"
    rc = P.main(["--gpus", "1", "--arch", "resnet50", "--dataset", "imagenet",
                 "--num-classes", "1000", "--record-size", "72", "--image-size", "64",
                 "--epochs", "1", "--batch-size", "16", "--n-train", "64", "--n-test", "32",
                 "--lr", "0.05", "--baseline-accuracy", "0", "--serving-dir", str(serving),
                 "--extra-args", json.dumps(["--steps=3", "--device-decode=1", "--workers=2"]),
                 "--spec", str(tmp_path / "spec.json")])
    assert rc == 0  # PIPELINE_STATE_SUCCEEDED
    devices, categories = [], []
    for root, _, files in os.walk(tmp_path):
        for fn in files:
            path = os.path.join(root, fn)
            if fn.endswith(".log"):
                with open(path) as f:
                    for line in f:
                        if "MIPIPE_METRICS" in line:
                            devices.append(json.loads(line.split("MIPIPE_METRICS", 1)[1])["device"])
            elif fn.endswith(".json") and os.path.getsize(path) < (64 << 20):
                with open(path) as f:
                    try:
                        doc = json.load(f)
                    except ValueError:
                        continue
                categories += [len(cm["annotationSpecs"]) for cm in _find(doc, "confusionMatrix")]
    assert devices and all(d.startswith("cuda") for d in devices), devices
    assert categories and set(categories) == {1000}, categories
    assert any("model.pth" in fs for _, _, fs in os.walk(serving))


def _write_rrc_dataset(data, size, num_classes, n_train, n_test):
    man = R.write_synthetic_dataset(str(data), "imagenet", n_train=n_train, n_test=n_test, seed=1,
                                    num_classes=num_classes, shape=(3, size, size), label_bytes=2)
    (data / "manifest.json").write_text(json.dumps(man))


def _run_task(tmp_path, data_dir, device_decode):
    from mipipe.launch.launcher import free_port
    out = tmp_path / f"run{device_decode}"
    env = dict(os.environ)
    for k in ("LOCAL_RANK", "GROUP_RANK"):
        env.pop(k, None)
    env.update({"WORLD_SIZE": "1", "RANK": "0", "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": str(free_port()), "HSA_ENABLE_IPC_MODE_LEGACY": "0",
                "PYTHONPATH": REPO + os.pathsep + env.get("PYTHONPATH", "")})
    args = ["--arch", "mnist_cnn", "--dataset", "imagenet", "--image-size", "32",
            "--data-dir", str(data_dir), "--batch_size", "64", "--num_epochs", "1", "--steps", "3",
            "--gpu", "0", "--local_training", "--model_dir", str(out), "--workers", "2",
            "--device-decode", str(device_decode), "--metrics-file", str(out / "metrics.json")]
    r = subprocess.run([sys.executable, "-m", "mipipe.train.task"] + args, env=env,
                       capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = json.loads((out / "metrics.json").read_text())
    assert m["steps"] == 3 and m["deterministic"] and m["device"].startswith("cuda"), m
    sd = torch.load(out / "resnet_distributed.pth", weights_only=True, map_location="cpu")
    return m, sd


def test_task_trains_identically_with_device_decode(tmp_path):
    """40x40 records with 2-byte labels -> 32x32 model input: the manifest selects rrc."""
    data = tmp_path / "data"
    _write_rrc_dataset(data, 40, 300, 320, 64)
    m0, sd0 = _run_task(tmp_path, data, 0)
    m1, sd1 = _run_task(tmp_path, data, 1)
    assert m0["loss"] == m1["loss"] and m0["loss"] == m0["loss"], (m0["loss"], m1["loss"])
    assert m0["accuracy"] == m1["accuracy"]
    assert list(sd0) == list(sd1) and len(sd0) > 0
    head = [v for v in sd0.values() if v.dim() == 2][-1]
    assert head.shape[0] == 300, "num_classes comes from the manifest"
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
