"""TrivialAugmentWide and Random Erasing of the record loaders: the integer definitions
(``records.reference_augment*``, ``reference_erase_box``) against Pillow, the literal tables against
their formulas, the native host loader against the definitions byte for byte, the loader's
options and the trainer flags on the CPU path.  The sample sets of the GPU tests
(tests/aug_common.py) are first shown to cover every op, sign, end bin and erase outcome."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from mipipe.data import records as R
from mipipe.runtime import runtime_available

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aug_common as AC  # noqa: E402

SEED = AC.SEED
OP = {name: k for k, name in enumerate(R.AUG_OPS)}


def _need_runtime():
    assert runtime_available(), "mipipe._runtime is not built"


# ------------------------------------------------------------------ the definitions themselves
def _pil_images():
    """uint8 [3, H, W] images of the three sizes: full range, a narrow range, few levels, and
    constant channels (AutoContrast's and Equalize's identity branches)."""
    rng = np.random.default_rng(0)
    out = []
    for H, W in ((32, 32), (17, 23), (9, 31)):
        out.append(rng.integers(0, 256, (3, H, W), dtype=np.uint8))
        out.append(rng.integers(60, 140, (3, H, W), dtype=np.uint8))
        out.append((rng.integers(0, 8, (3, H, W)) * rng.integers(0, 30, (3, 1, 1))
                    + rng.integers(0, 40, (3, 1, 1))).clip(0, 255).astype(np.uint8))
        flat = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
        flat[1] = 77          # one level: Equalize and AutoContrast keep the channel
        flat[2, :, :] = 5
        flat[2, 0, 0] = 9     # two levels, the last bin holding all but H*W - 1 < 255 pixels: step 0
        out.append(flat)
    return out


def test_reference_agrees_with_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageOps

    def pil(img):
        return Image.fromarray(np.transpose(img, (1, 2, 0)))

    def unpil(im):
        return np.transpose(np.asarray(im), (2, 0, 1))

    def close(a, b, tol, what):
        d = int(np.abs(a.astype(int) - b.astype(int)).max())
        assert d <= tol, (what, d)

    identity = {"AutoContrast": 0, "Equalize": 0}
    for img in _pil_images():
        P = pil(img)
        for m in (0, 1, 3, 7, 10, 15, 19, 22, 26, 29, 30):
            for sign in (1, -1):
                f = 1 + sign * 0.99 * m / 30
                for name, enh in (("Brightness", ImageEnhance.Brightness),
                                  ("Color", ImageEnhance.Color),
                                  ("Contrast", ImageEnhance.Contrast),
                                  ("Sharpness", ImageEnhance.Sharpness)):
                    close(R.reference_augment_op(img, OP[name], m, sign), unpil(enh(P).enhance(f)),
                          1, (name, m, sign, img.shape))  # Pillow truncates where we round
            bits = 8 - int(round(m / 5))
            close(R.reference_augment_op(img, OP["Posterize"], m, 1),
                  unpil(ImageOps.posterize(P, bits)), 0, ("Posterize", m))
            close(R.reference_augment_op(img, OP["Solarize"], m, -1),
                  unpil(ImageOps.solarize(P, 255 - 8.5 * m)), 0, ("Solarize", m))
        ac = R.reference_augment_op(img, OP["AutoContrast"], 0, 1)
        close(ac, unpil(ImageOps.autocontrast(P)), 1, "AutoContrast")
        eq = R.reference_augment_op(img, OP["Equalize"], 0, 1)
        close(eq, unpil(ImageOps.equalize(P)), 0, "Equalize")
        for name, res in (("AutoContrast", ac), ("Equalize", eq)):
            identity[name] += sum(np.array_equal(res[c], img[c]) for c in range(3))
    assert identity["AutoContrast"] >= 3 and identity["Equalize"] >= 6, identity


def test_translate_is_roll_and_zero_and_identity_ops():
    rng = np.random.default_rng(1)
    for shape in ((3, 32, 32), (3, 17, 23), (1, 9, 31)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        C, H, W = shape
        for m in range(31):
            for sign in (1, -1):
                t = sign * ((32 * m) // 30)  # the image moves by +t pixels
                for name, axis, ext in (("TranslateX", 2, W), ("TranslateY", 1, H)):
                    want = np.roll(img, t, axis=axis)
                    sl = [slice(None)] * 3
                    sl[axis] = slice(0, min(t, ext)) if t >= 0 else slice(max(ext + t, 0), ext)
                    want[tuple(sl)] = 0
                    got = R.reference_augment_op(img, OP[name], m, sign)
                    assert np.array_equal(got, want), (name, m, sign, shape)
        for name in ("Identity", "ShearX", "ShearY", "Rotate", "Brightness", "Color", "Contrast",
                     "Sharpness", "Posterize", "TranslateX", "TranslateY"):  # Solarize maps 255 to 0
            assert np.array_equal(R.reference_augment_op(img, OP[name], 0, 1), img), name
    img = rng.integers(0, 256, (3, 16, 16), dtype=np.uint8)
    # Rotate at bin 20 is a quarter turn (cos 0, sin 1): exact on a square image
    assert np.array_equal(R.reference_augment_op(img, OP["Rotate"], 20, 1),
                          np.rot90(img, -1, axes=(1, 2)))
    assert np.array_equal(R.reference_augment_op(img, OP["Rotate"], 20, -1),
                          np.rot90(img, 1, axes=(1, 2)))
    with pytest.raises(ValueError):
        R.reference_augment_op(np.zeros((2, 4, 4), np.uint8), 0, 0, 1)


def test_literal_tables_equal_the_formulas():
    assert list(R.COS_Q16) == [round(65536 * math.cos(math.radians(4.5 * m))) for m in range(31)]
    assert list(R.SIN_Q16) == [round(65536 * math.sin(math.radians(4.5 * m))) for m in range(31)]
    assert list(R.ERASE_RATIO_Q16) == [round(65536 * 0.3 * 11 ** (t / 63)) for t in range(64)]
    assert (R.ERASE_RATIO_Q16[0], R.ERASE_RATIO_Q16[31], R.ERASE_RATIO_Q16[63]) == \
        (19661, 63978, 216269)


def test_params_and_force_word():
    a = R._splitmix64(R._sample_word(SEED, 1, 45) ^ 0x5441776964654F70)
    assert R.reference_augment_params(SEED, 1, 45) == (
        ((a & 0xFFFFFFFF) * 14) >> 32, (((a >> 32) & 0xFFFFFF) * 31) >> 24,
        1 if (a >> 60) & 1 else -1)
    for op in range(14):
        for m in (0, 30):
            for sign in (1, -1):
                f = R.augment_force(op, m, sign)
                assert f == op | m << 8 | (sign > 0) << 16
                assert R.reference_augment_params(SEED, 0, 3, f) == (op, m, sign)
    assert R.augment_force("Equalize", 3, -1) == 13 | 3 << 8
    for bad in (14, 31 << 8, 1 << 17):
        with pytest.raises(ValueError):
            R.reference_augment_params(0, 0, 0, bad)
    assert R.erase_pq(0.0) == 0 and R.erase_pq(1.0) == 1 << 24 and R.erase_pq(0.1) == 1677722


# ------------------------------------------------------------------ the GPU tests' sample sets
@pytest.mark.parametrize("shape,lb", AC.RANDOM_SETS, ids=AC.SHAPE_IDS[:3])
def test_policy_sample_sets_cover_every_op(shape, lb):
    AC.assert_policy_coverage(AC.policy_draws(shape, AC.N_RANDOM, lb))


def test_erase_sample_sets_cover_every_outcome():
    draws = {out: AC.erase_draws((3, *out), AC.N_RANDOM, out, AC.PQ_HALF) for out in AC.ERASE_OUTS}
    AC.assert_erase_coverage(draws)
    for out in AC.ERASE_OUTS:  # p = 0 never applies, p = 1 always
        assert all(d[4] == -1 for d in AC.erase_draws((3, *out), AC.N_RANDOM, out, 0))
        assert all(d[4] != -1 for d in AC.erase_draws((3, *out), AC.N_RANDOM, out, 1 << 24))
    # a row of the 32x32 fp32 / bf16 output whose box does not start on a 16-byte boundary
    assert any(k >= 0 and x0 % 4 and x0 % 8 for _, x0, _, _, k in draws[(32, 32)])


def test_forced_sets_contain_the_special_images():
    for shape, lb, n, _ in AC.SHAPES:
        _, img, _, _ = AC.dataset(shape, n, lb)
        assert any(img[i].min() == img[i].max() for i in range(n)), "a constant image"
        assert any(len(np.unique(img[i])) <= 24 for i in range(n)), "a few-level image"


# ------------------------------------------------------------------ loaders
def _files(tmp_path, shape, n, label_bytes=1):
    _, img, lab, _ = AC.dataset(shape, n, label_bytes)
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


LOADER_CASES = [((3, 32, 32), 1, "crop", None), ((3, 32, 32), 1, "rrc", (24, 24)),
                ((1, 28, 28), 1, "crop", None), ((1, 28, 28), 1, "rrc", (5, 7)),
                ((3, 17, 23), 2, "crop", None), ((3, 17, 23), 2, "rrc", (3, 40))]


@pytest.mark.parametrize("no_native", [False, True], ids=["native", "python"])
@pytest.mark.parametrize("shape,lb,transform,out", LOADER_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-{c[2]}" for c in LOADER_CASES])
def test_loader_equals_reference(tmp_path, monkeypatch, shape, lb, transform, out, no_native):
    """Augmentation and erase on, both transforms, epochs 0 and 1: the native host loader (and
    the pure-Python twin, and decode="device" on the CPU device) give the bytes of augment -> crop /
    rrc -> erase in NumPy; fp32 compared as uint32."""
    if no_native:
        monkeypatch.setenv("MIPIPE_NO_NATIVE_RUNTIME", "1")
    else:
        _need_runtime()
    n = 64
    files, img, lab = _files(tmp_path, shape, n, lb)
    C = shape[0]
    kw = dict(transform=transform, out_size=out) if transform == "rrc" else {}
    res = {}
    for decode in ("host", "device"):
        dl = R.RecordDataLoader(files, shape, batch_size=7, train=True, seed=SEED, workers=3,
                                prefetch=2, decode=decode, mean=AC.MEANS[C], std=AC.STDS[C],
                                label_bytes=lb, auto_augment="ta_wide", random_erase=0.5, **kw)
        assert dl.native == (not no_native)
        res[decode] = _epochs(dl)
    xh, yh, order = res["host"]
    xd, yd, _ = res["device"]
    ref = np.stack([AC.transform_reference(img[i], i, e, shape, transform, out, True, AC.PQ_HALF)
                    for e in (0, 1) for i in order[e]])
    assert xh.dtype == torch.float32 and tuple(xh.shape) == ref.shape
    assert np.array_equal(xh.numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(xd.numpy().view(np.uint32), ref.view(np.uint32))
    labs = torch.from_numpy(np.concatenate([lab[order[0]], lab[order[1]]]))
    assert torch.equal(yh, labs) and torch.equal(yd, labs)
    assert (ref == 0).any() and not np.array_equal(ref[:n], ref[n:])


def test_native_loader_each_option_alone(tmp_path):
    _need_runtime()
    shape, n = (3, 17, 23), 64
    files, img, _ = _files(tmp_path, shape, n)
    for aa, p in (("ta_wide", 0.0), (None, 1.0)):
        dl = R.RecordDataLoader(files, shape, batch_size=9, train=True, seed=SEED, workers=2,
                                mean=AC.MEANS[3], std=AC.STDS[3], auto_augment=aa, random_erase=p)
        x, _, order = _epochs(dl, (1,))
        ref = np.stack([AC.transform_reference(img[i], i, 1, shape, "crop", None, aa,
                                               R.erase_pq(p)) for i in order[0]])
        assert np.array_equal(x.numpy().view(np.uint32), ref.view(np.uint32)), (aa, p)


def test_same_seed_same_batches_and_eval_untouched(tmp_path):
    shape, n = (3, 32, 32), 64
    files, _, _ = _files(tmp_path, shape, n)
    kw = dict(batch_size=16, seed=SEED, workers=2, mean=AC.MEANS[3], std=AC.STDS[3])
    on = dict(auto_augment="ta_wide", random_erase=0.5)
    a, ya, _ = _epochs(R.RecordDataLoader(files, shape, train=True, **kw, **on))
    b, yb, _ = _epochs(R.RecordDataLoader(files, shape, train=True, **kw, **on))
    assert torch.equal(a, b) and torch.equal(ya, yb)
    assert not torch.equal(a[:n], a[n:]), "another epoch differs"
    plain, _, _ = _epochs(R.RecordDataLoader(files, shape, train=True, **kw))
    assert not torch.equal(a, plain)
    for decode in ("host", "device"):
        ev, _, _ = _epochs(R.RecordDataLoader(files, shape, train=False, decode=decode, **kw, **on))
        ev0, _, _ = _epochs(R.RecordDataLoader(files, shape, train=False, decode=decode, **kw))
        assert torch.equal(ev, ev0), "train=False ignores both options"
    dl = R.RecordDataLoader(files, shape, train=False, **kw, **on)
    assert dl.auto_augment is None and dl.erase_pq == 0


def test_argument_validation(tmp_path):
    shape, n = (3, 32, 32), 64
    files, _, _ = _files(tmp_path, shape, n)
    for bad in ({"auto_augment": "randaugment"}, {"auto_augment": "TA_WIDE"},
                {"random_erase": -0.1}, {"random_erase": 1.5}):
        with pytest.raises(ValueError):
            R.RecordDataLoader(files, shape, 8, **bad)
    with pytest.raises(ValueError):  # two channels have no grey value
        R.RecordDataLoader(files, (2, 48, 32), 8, auto_augment="ta_wide")
    R.RecordDataLoader(files, shape, 8, auto_augment=None, random_erase=0.0)
    R.RecordDataLoader(files, shape, 8, auto_augment="none", random_erase=1.0)
    if runtime_available():
        from mipipe.runtime import runtime
        cfg = runtime().LoaderConfig()
        cfg.files, cfg.mean, cfg.std = files, [0.0] * 3, [1.0] * 3
        assert cfg.auto_augment == "" and cfg.erase_pq == 0
        cfg.auto_augment = "rand"
        with pytest.raises(ValueError):
            runtime().RecordLoader(cfg)
        cfg.auto_augment, cfg.erase_pq = "ta_wide", (1 << 24) + 1
        with pytest.raises(ValueError):
            runtime().RecordLoader(cfg)


def test_ref_kernels_follow_the_definitions():
    from mipipe.ops import kernels as K
    shape, lb, n, _ = AC.SHAPES[3]
    rec, img, lab, gidx = AC.dataset(shape, n, lb)
    r, g = torch.from_numpy(rec.copy()), torch.from_numpy(gidx.copy())
    out = K.record_augment(r, g, shape, SEED, 1, lb).numpy()
    assert np.array_equal(out[:, :lb], rec[:, :lb])
    assert np.array_equal(out[:, lb:].reshape(n, *shape), AC.random_reference(shape, n, lb, 1))
    f = R.augment_force("Rotate", 7, -1)
    out = K.record_augment(r, g, shape, SEED, 1, lb, force=f).numpy()
    assert np.array_equal(out[:, lb:].reshape(n, *shape),
                          AC.forced_reference(shape, n, lb, OP["Rotate"], 7, -1))
    x = torch.randn(n, 3, 5, 7)
    want = AC.erase_reference(x.numpy(), gidx, 0, AC.PQ_HALF)
    assert K.batch_erase_(x, g, SEED, 0, AC.PQ_HALF) is x
    assert np.array_equal(x.numpy().view(np.uint32), want.view(np.uint32))


def test_task_trains_with_both_flags_on_cpu(tmp_path, monkeypatch, capsys):
    import mipipe.train.task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    data = tmp_path / "data"
    man = R.write_synthetic_dataset(str(data), "cifar10", n_train=64, n_test=32, seed=1)
    (data / "manifest.json").write_text(json.dumps(man))
    out = tmp_path / "out"
    args = ["--arch", "mnist_cnn", "--dataset", "cifar10", "--data-dir", str(data),
            "--batch_size", "32", "--num_epochs", "1", "--local_training", "--model_dir", str(out),
            "--log-every", "0", "--workers", "2", "--metrics-file", str(tmp_path / "m.json"),
            "--auto-augment", "ta_wide", "--random-erase", "0.25"]
    assert T.main(args) == 0
    m = json.loads((tmp_path / "m.json").read_text())
    assert m["steps"] == 2 and m["loss"] == m["loss"]
    assert m["auto_augment"] == "ta_wide" and m["random_erase"] == 0.25
    assert "auto_augment=ta_wide random_erase=0.25" in capsys.readouterr().out
    a = T.build_parser().parse_args([])
    assert a.auto_augment == "none" and a.random_erase == 0.0
    with pytest.raises(SystemExit, match="--data-dir"):  # synthetic data is not augmented
        T.main(["--arch", "mnist_cnn", "--local_training", "--auto-augment", "ta_wide",
                "--model_dir", str(out)])
    with pytest.raises(SystemExit):
        T.main(args[:-1] + ["1.5"])
