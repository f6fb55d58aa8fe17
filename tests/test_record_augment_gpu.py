"""TrivialAugmentWide and Random Erasing on the MI355X (csrc/kernels/augment.hip).

``record_augment`` and ``batch_erase_`` must reproduce ``records.reference_augment`` and
``reference_erase_box`` — the NumPy definitions the host loader matches byte for byte
(test_record_augment_cpu.py) — exactly: bytes against bytes, fp32 as uint32 words, bf16 as uint16
words.  The sample sets are tests/aug_common.py's, whose coverage the CPU tests show."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mipipe.data import records as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_common as AC  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = AC.SEED
DEV = torch.device("cuda", 0)


def _native():
    from mipipe.ops._native import load_error, native, native_available
    assert native_available(), f"mipipe._C not loadable: {load_error()!r}"
    return native()


def _augment(rec, gidx, shape, lb, epoch, batch, force=-1, parts=0):
    """The native kernel over the set in batches of ``batch`` (the last one partial)."""
    nat = _native()
    outs = []
    for b in range(0, len(rec), batch):
        r = torch.from_numpy(rec[b:b + batch].copy()).to(DEV)
        g = torch.from_numpy(gidx[b:b + batch].copy()).to(DEV)
        outs.append(nat.record_augment(r, g, *shape, SEED, epoch, lb, force, parts))
    return torch.cat(outs).cpu().numpy()


@pytest.mark.parametrize("op", range(len(R.AUG_OPS)), ids=R.AUG_OPS)
@pytest.mark.parametrize("shape,lb,n,batch", AC.SHAPES, ids=AC.SHAPE_IDS)
def test_forced_op_equals_reference(shape, lb, n, batch, op):
    """Every op x m in {0, 1, 15, 30} x both signs, batches of 7 out of 20 records."""
    rec, _, _, gidx = AC.dataset(shape, n, lb)
    for m in AC.MAGNITUDES:
        for sign in (1, -1):
            got = _augment(rec, gidx, shape, lb, 0, batch, R.augment_force(op, m, sign))
            assert got.shape == rec.shape and got.dtype == np.uint8
            assert np.array_equal(got[:, :lb], rec[:, :lb]), "labels are intact"
            ref = AC.forced_reference(shape, n, lb, op, m, sign)
            bad = np.argwhere(got[:, lb:].reshape(ref.shape) != ref)
            assert bad.size == 0, (R.AUG_OPS[op], m, sign, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("shape,lb", AC.RANDOM_SETS, ids=AC.SHAPE_IDS[:3])
def test_random_policy_equals_reference(shape, lb):
    n = AC.N_RANDOM
    AC.assert_policy_coverage(AC.policy_draws(shape, n, lb))
    rec, _, _, gidx = AC.dataset(shape, n, lb)
    for epoch in (0, 1):
        ref = AC.random_reference(shape, n, lb, epoch)
        for parts in (0, 3):  # blocks per sample: by size, and several (the reduction is redone)
            got = _augment(rec, gidx, shape, lb, epoch, 7, parts=parts)
            assert np.array_equal(got[:, :lb], rec[:, :lb])
            bad = np.argwhere(got[:, lb:].reshape(ref.shape) != ref)
            assert bad.size == 0, (epoch, parts, len(bad), bad[:4].tolist())
    assert not np.array_equal(AC.random_reference(shape, n, lb, 0),
                              AC.random_reference(shape, n, lb, 1))


def test_augment_misaligned_source():
    """A record tensor that starts at an odd address: source and destination do not share their
    alignment, so the table path reads bytes."""
    nat = _native()
    shape, lb, n, _ = AC.SHAPES[0]
    rec, _, _, gidx = AC.dataset(shape, n, lb)
    buf = torch.zeros(rec.size + 1, dtype=torch.uint8, device=DEV)
    r = buf[1:].view(n, -1)
    r.copy_(torch.from_numpy(rec.copy()))
    g = torch.from_numpy(gidx.copy()).to(DEV)
    for name in ("Equalize", "Solarize", "Color"):
        got = nat.record_augment(r, g, *shape, SEED, 0, lb, R.augment_force(name, 15, 1), 0)
        ref = AC.forced_reference(shape, n, lb, R.AUG_OPS.index(name), 15, 1)
        assert np.array_equal(got.cpu().numpy()[:, lb:].reshape(ref.shape), ref), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("out", AC.ERASE_OUTS, ids=["32x32", "5x7", "3x40"])
def test_batch_erase_equals_reference(out, dtype):
    nat = _native()
    n = AC.N_RANDOM
    _, _, _, gidx = AC.dataset((3, *out), n)
    word = np.uint32 if dtype == torch.float32 else np.uint16
    wt = torch.int32 if dtype == torch.float32 else torch.int16
    torch.manual_seed(sum(out))
    x0 = torch.randn(n, 3, *out).to(dtype)
    x0[x0 == 0] = 1  # no zero outside a box
    words = x0.view(wt).numpy().view(word)
    for p in (0.0, 0.5, 1.0):
        pq = R.erase_pq(p)
        for epoch in (0, 1):
            want = AC.erase_reference(words, gidx, epoch, pq)
            xs = []
            for b in range(0, n, 7):
                x = x0[b:b + 7].to(DEV)
                g = torch.from_numpy(gidx[b:b + 7].copy()).to(DEV)
                assert nat.batch_erase_(x, g, SEED, epoch, pq).data_ptr() == x.data_ptr()
                xs.append(x)
            got = torch.cat(xs).cpu().view(wt).numpy().view(word)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (p, epoch, len(bad), bad[:4].tolist())
            if p == 0.0:
                assert np.array_equal(got, words), "p = 0 leaves every bit"
            else:
                assert (got == 0).any()


def test_bindings_reject_bad_arguments():
    nat = _native()
    rec = torch.zeros(2, 193, dtype=torch.uint8, device=DEV)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    ok = (3, 8, 8, SEED, 0, 1)
    out = nat.record_augment(rec, idx, *ok)
    assert out.data_ptr() != rec.data_ptr() and tuple(out.shape) == (2, 193)
    assert tuple(nat.record_augment(rec[:0], idx[:0], *ok).shape) == (0, 193)
    for args in ((rec.cpu(), idx, *ok), (rec, idx.int(), *ok), (rec, idx[:1], *ok),
                 (rec.int(), idx, *ok), (rec, idx, 3, 8, 8, SEED, 0, 2),
                 (rec, idx, 3, 8, 8, SEED, 0, 1, 14), (rec, idx, 3, 8, 8, SEED, 0, 1, 31 << 8),
                 (rec, idx, 3, 8, 8, SEED, 0, 1, -1, 65),
                 (torch.zeros(2, 129, dtype=torch.uint8, device=DEV), idx, 2, 8, 8, SEED, 0, 1)):
        with pytest.raises(RuntimeError):
            nat.record_augment(*args)
    x = torch.ones(2, 3, 8, 8, device=DEV)
    for args in ((x.cpu(), idx, SEED, 0, 1), (x, idx.cpu(), SEED, 0, 1), (x, idx[:1], SEED, 0, 1),
                 (x.half(), idx, SEED, 0, 1), (x[0], idx, SEED, 0, 1), (x, idx, SEED, 0, -1),
                 (x, idx, SEED, 0, (1 << 24) + 1)):
        with pytest.raises(RuntimeError):
            nat.batch_erase_(*args)
    empty = torch.ones(0, 3, 8, 8, device=DEV)
    assert nat.batch_erase_(empty, idx[:0], SEED, 0, 1 << 24).numel() == 0


@pytest.mark.parametrize("transform,out", [("crop", None), ("rrc", (24, 24))], ids=["crop", "rrc"])
def test_loader_device_decode_equals_host(tmp_path, transform, out):
    _native()
    shape, n = (3, 32, 32), AC.N_RANDOM
    _, img, lab, _ = AC.dataset(shape, n)
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    R.write_records(files[0], img[:20], lab[:20])
    R.write_records(files[1], img[20:], lab[20:])
    kw = dict(transform="rrc", out_size=out) if transform == "rrc" else {}
    res = {}
    for decode in ("host", "device"):
        dl = R.RecordDataLoader(files, shape, batch_size=9, train=True, seed=SEED, workers=3,
                                prefetch=2, device="cuda", decode=decode, mean=AC.MEANS[3],
                                std=AC.STDS[3], auto_augment="ta_wide", random_erase=0.5, **kw)
        assert dl.native
        dl.set_epoch(1)
        batches = list(dl)
        assert [len(y) for _, y in batches] == [9] * 7 + [1]
        res[decode] = (torch.cat([x for x, _ in batches]), torch.cat([y for _, y in batches]))
    (xh, yh), (xd, yd) = res["host"], res["device"]
    assert xd.is_cuda and xd.dtype == torch.float32
    assert torch.equal(xd.view(torch.int32), xh.view(torch.int32)) and torch.equal(yd, yh)
    order = list(iter(dl.sampler))
    ref = np.stack([AC.transform_reference(img[i], i, 1, shape, transform, out, True, AC.PQ_HALF)
                    for i in order])
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _run_task(tmp_path, data_dir, device_decode):
    from mipipe.launch.launcher import free_port
    out = tmp_path / f"run{device_decode}"
    env = dict(os.environ)
    for k in ("LOCAL_RANK", "GROUP_RANK"):
        env.pop(k, None)
    env.update({"WORLD_SIZE": "1", "RANK": "0", "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": str(free_port()), "HSA_ENABLE_IPC_MODE_LEGACY": "0",
                "PYTHONPATH": REPO + os.pathsep + env.get("PYTHONPATH", "")})
    args = ["--arch", "resnet18", "--dataset", "cifar10", "--data-dir", str(data_dir),
            "--batch_size", "16", "--num_epochs", "1", "--steps", "3", "--log-every", "1",
            "--gpu", "0", "--local_training", "--model_dir", str(out), "--workers", "2",
            "--device-decode", str(device_decode), "--auto-augment", "ta_wide",
            "--random-erase", "0.5", "--metrics-file", str(out / "metrics.json")]
    r = subprocess.run([sys.executable, "-m", "mipipe.train.task"] + args, env=env,
                       capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = json.loads((out / "metrics.json").read_text())
    assert m["steps"] == 3 and m["deterministic"] and m["device"].startswith("cuda"), m
    assert m["auto_augment"] == "ta_wide" and m["random_erase"] == 0.5
    assert "auto_augment=ta_wide random_erase=0.5" in r.stdout
    sd = torch.load(out / "resnet_distributed.pth", weights_only=True, map_location="cpu")
    return m, sd


def test_task_trains_identically_with_device_decode(tmp_path):
    """3 ResNet-18 steps on 64 CIFAR-shaped records, both options on: the same loss and the same
    weights whether the host loader or the kernels augment."""
    data = tmp_path / "data"
    man = R.write_synthetic_dataset(str(data), "cifar10", n_train=64, n_test=32, seed=1)
    (data / "manifest.json").write_text(json.dumps(man))
    m0, sd0 = _run_task(tmp_path, data, 0)
    m1, sd1 = _run_task(tmp_path, data, 1)
    assert m0["loss"] == m1["loss"] and m0["loss"] == m0["loss"], (m0["loss"], m1["loss"])
    assert m0["accuracy"] == m1["accuracy"]
    assert list(sd0) == list(sd1) and len(sd0) > 0
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k
