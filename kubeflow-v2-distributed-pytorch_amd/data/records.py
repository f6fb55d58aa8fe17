"""Binary image-record datasets + the native multi-threaded loader.

Record layout = CIFAR-10 binary (``[label byte][C planes of H*W uint8]``, 3073 bytes for
32x32x3), the format ``torchvision.datasets.CIFAR10`` downloads and task.py decodes
(task.py:246-263).  There is no network here, so the pipeline's *preprocess* step writes such
files from a deterministic, learnable generator (:func:`write_synthetic_dataset`); the *train*
and *eval* steps read them through :class:`RecordDataLoader`, which drives the C++
``RecordLoader`` (csrc/runtime/loader.cpp: memory-mapped files, worker threads, RandomCrop
(padding) + RandomHorizontalFlip + Normalize, ordered prefetch ring) and hands each batch to the
GPU through a pinned staging buffer and one non-blocking copy.  With ``decode="device"`` the
loader threads only gather the uint8 records; those are uploaded as they are and the same
transform runs on the GPU (csrc/kernels/records.hip), bit-identical to the host path.  Labels are
1 byte as in CIFAR-10, or ``label_bytes`` (up to 8) little-endian bytes.

:func:`reference_transform` is the plain-NumPy definition of the per-sample transform the
native loader implements (tests compare the two bit-for-bit).

A second transform, ``transform="rrc"``, resizes: RandomResizedCrop + flip + Normalize in
training and a 7/8 centre crop in evaluation, from the stored size to any ``out_size`` (256x256
records -> 224x224 batches).  Its geometry is integer-only, so :func:`reference_transform_rrc`,
the native loader and the device kernel give the same bits.
"""
from __future__ import annotations

import math
import os
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from mipipe.parallel.sampler import DistributedSampler

__all__ = ["write_records", "read_records", "write_synthetic_dataset", "reference_transform",
           "reference_rrc_box", "reference_transform_rrc", "RATIO_Q16", "RecordDataLoader",
           "reference_augment_params", "reference_augment_op", "reference_augment",
           "reference_erase_box", "augment_force", "erase_pq", "AUG_OPS", "AUG_POLICIES",
           "COS_Q16", "SIN_Q16", "ERASE_RATIO_Q16",
           "CIFAR10_MEAN", "CIFAR10_STD", "IMAGENET_MEAN", "IMAGENET_STD", "dataset_files"]

# task.py:249-251
CIFAR10_MEAN = (0.4914, 0.4822, 0.4465)
CIFAR10_STD = (0.2023, 0.1994, 0.2010)
MNIST_MEAN = (0.1307,)
MNIST_STD = (0.3081,)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

_MASK64 = (1 << 64) - 1


def _check_label_bytes(label_bytes: int) -> int:
    if not 1 <= int(label_bytes) <= 8:
        raise ValueError(f"label_bytes must be in [1, 8], got {label_bytes}")
    return int(label_bytes)


def write_records(path: str, images: np.ndarray, labels: np.ndarray, label_bytes: int = 1) -> None:
    """images uint8 [N, C, H, W], labels [N] (< 256 ** label_bytes, stored little-endian) ->
    CIFAR-binary record file (``label_bytes`` = 1 is the CIFAR-10 layout)."""
    rec = _pack_records(images, labels, label_bytes)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    rec.tofile(path)


def _pack_records(images: np.ndarray, labels: np.ndarray, label_bytes: int) -> np.ndarray:
    lb = _check_label_bytes(label_bytes)
    images = np.ascontiguousarray(images, dtype=np.uint8)
    n = images.shape[0]
    labels = np.asarray(labels).astype(np.int64).reshape(n)
    if n and (labels.min() < 0 or (lb < 8 and labels.max() >= 1 << (8 * lb))):
        raise ValueError(f"labels do not fit {lb} byte(s)")
    rec = np.empty((n, lb + int(np.prod(images.shape[1:]))), dtype=np.uint8)
    for k in range(lb):
        rec[:, k] = (labels >> (8 * k)) & 0xFF
    rec[:, lb:] = images.reshape(n, -1)
    return rec


def _decode_labels(raw: np.ndarray, label_bytes: int) -> np.ndarray:
    y = np.zeros(raw.shape[0], dtype=np.int64)
    for k in range(label_bytes):
        y |= raw[:, k].astype(np.int64) << (8 * k)
    return y


def read_records(path: str, shape: Sequence[int], label_bytes: int = 1
                 ) -> Tuple[np.ndarray, np.ndarray]:
    C, H, W = shape
    lb = _check_label_bytes(label_bytes)
    raw = np.fromfile(path, dtype=np.uint8).reshape(-1, lb + C * H * W)
    return raw[:, lb:].reshape(-1, C, H, W), _decode_labels(raw, lb)


def write_synthetic_dataset(out_dir: str, name: str = "cifar10", n_train: int = 10000,
                            n_test: int = 2000, seed: int = 0, num_classes: int = 10,
                            shape: Optional[Sequence[int]] = None, label_bytes: int = 1) -> dict:
    """Learnable synthetic dataset in CIFAR-binary layout: class template (low-frequency
    pattern) + per-sample noise, quantised to uint8.  ``shape`` (C, H, W) overrides the shape
    ``name`` stands for (``imagenet``: 256x256 stored, for the ``"rrc"`` transform to resize).
    Written in chunks of a few MB of float64 work, so neither the class templates nor the
    images are ever held whole.  Returns a manifest dict."""
    shape = (tuple(int(v) for v in shape) if shape is not None
             else {"cifar10": (3, 32, 32), "mnist": (1, 28, 28), "imagenet": (3, 256, 256)}[name])
    C, H, W = shape
    lb = _check_label_bytes(label_bytes)
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, 1.0, size=(num_classes, C, -(-H // 4), -(-W // 4)))
    chunk = max(1, (1 << 21) // (C * H * W))  # <= 16 MB of float64 per temporary

    files = {}
    os.makedirs(out_dir, exist_ok=True)
    for split, n, s in (("train", n_train, 1), ("test", n_test, 2)):
        r = np.random.default_rng(seed * 1000 + s)
        y = r.integers(0, num_classes, size=n)
        path = os.path.join(out_dir, f"{name}_{split}.bin")
        with open(path, "wb") as f:
            # the generator fills draws in order, so chunked draws are the one-call stream
            for a in range(0, n, chunk):
                yc = y[a:a + chunk]
                templates = np.kron(base[yc], np.ones((1, 1, 4, 4)))[:, :, :H, :W]
                x = 0.8 * templates + r.normal(0.0, 1.0, size=(len(yc), C, H, W))
                img = np.clip(x * 40.0 + 128.0, 0, 255).astype(np.uint8)
                _pack_records(img, yc, lb).tofile(f)
        files[split] = path
    return {"name": name, "shape": list(shape), "num_classes": num_classes,
            "label_bytes": int(label_bytes), "n_train": n_train, "n_test": n_test, "files": files}


def dataset_files(data_dir: str, name: str, split: str) -> List[str]:
    """Record files of ``split`` in ``data_dir``: our ``<name>_<split>.bin`` or the original
    CIFAR-10 binary names (data_batch_*.bin / test_batch.bin)."""
    own = os.path.join(data_dir, f"{name}_{split}.bin")
    if os.path.exists(own):
        return [own]
    if name == "cifar10":
        d = os.path.join(data_dir, "cifar-10-batches-bin")
        d = d if os.path.isdir(d) else data_dir
        names = ([f"data_batch_{i}.bin" for i in range(1, 6)] if split == "train"
                 else ["test_batch.bin"])
        found = [os.path.join(d, n) for n in names if os.path.exists(os.path.join(d, n))]
        if found:
            return found
    return []


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def reference_transform(img: np.ndarray, index: int, epoch: int, seed: int, train: bool,
                        pad: int, flip: bool, mean, std) -> np.ndarray:
    """NumPy definition of loader.cpp's per-sample transform (uint8 CHW -> float32 CHW)."""
    C, H, W = img.shape
    dy = dx = 0
    fl = False
    if train:
        h = _splitmix64(seed ^ _splitmix64(((epoch * 0x100000001B3) & _MASK64) ^ index))
        if pad > 0:
            dy = int(h % (2 * pad + 1)) - pad
            dx = int((h >> 16) % (2 * pad + 1)) - pad
        fl = flip and bool((h >> 40) & 1)
    padded = np.zeros((C, H + 2 * pad, W + 2 * pad), dtype=np.float32)
    padded[:, pad:pad + H, pad:pad + W] = img
    out = padded[:, pad + dy:pad + dy + H, pad + dx:pad + dx + W]
    if fl:
        out = out[:, :, ::-1]
    m = np.asarray(mean, np.float32)[:, None, None]
    s = np.asarray(std, np.float32)[:, None, None]
    return (out * (1.0 / (255.0 * s)) + (-m / s)).astype(np.float32)


# The "rrc" transform (csrc/common/rrc.hpp holds the native copy of the geometry): aspect ratios
# w/h in Q16, round(65536 * 0.75 * (16/9) ** (t/63)), log-uniform over [3/4, 4/3].
RATIO_Q16 = (
    49152, 49603, 50058, 50517, 50981, 51449, 51921, 52397, 52878, 53363, 53852, 54346, 54845,
    55348, 55856, 56368, 56886, 57407, 57934, 58466, 59002, 59543, 60090, 60641, 61197, 61759,
    62325, 62897, 63474, 64057, 64644, 65237, 65836, 66440, 67050, 67665, 68285, 68912, 69544,
    70182, 70826, 71476, 72132, 72793, 73461, 74135, 74815, 75502, 76195, 76894, 77599, 78311,
    79030, 79755, 80486, 81225, 81970, 82722, 83481, 84247, 85020, 85800, 86587, 87381)
RRC_MAX_EXTENT = 32768  # stored and output extents: keeps every Q16 product inside 64 bits


def _check_rrc_geometry(H: int, W: int, Ho: int, Wo: int) -> None:
    if min(H, W) < 2 or min(Ho, Wo) < 1 or max(H, W, Ho, Wo) > RRC_MAX_EXTENT:
        raise ValueError(f"rrc needs stored extents in [2, {RRC_MAX_EXTENT}] and output extents "
                         f"in [1, {RRC_MAX_EXTENT}], got {(H, W)} -> {(Ho, Wo)}")


def reference_rrc_box(seed: int, epoch: int, index: int, H: int, W: int, train: bool,
                      flip: bool = True) -> Tuple[int, int, int, int, int]:
    """(y0, x0, h, w, flip): the source box of the ``"rrc"`` transform, integers only.
    Training: RandomResizedCrop(scale 0.08-1, ratio 3/4-4/3), ten attempts keyed by splitmix64 of
    (seed, epoch, index) — the crop transform's word, whose bit 40 is the flip — then the centred
    ratio-clamped fallback.  Evaluation: the centre square of 7/8 of the short side."""
    if not train:
        s = (min(H, W) * 7) // 8
        return (H - s) // 2, (W - s) // 2, s, s, 0
    h0 = _splitmix64(seed ^ _splitmix64(((epoch * 0x100000001B3) & _MASK64) ^ (index & _MASK64)))
    fl = int(bool(flip) and ((h0 >> 40) & 1))
    for k in range(10):
        g = _splitmix64((h0 + k + 1) & _MASK64)
        sq = 5243 + (((65536 - 5243) * (g & 0xFFFFFF)) >> 24)  # scale in Q16 over [0.08, 1)
        area = (H * W * sq) >> 16
        r = RATIO_Q16[(g >> 24) & 63]
        w = math.isqrt((area * r) >> 16)
        h = math.isqrt((area << 16) // r)
        if 0 < w <= W and 0 < h <= H:
            g2 = _splitmix64(g)
            return (g2 & 0xFFFFFFFF) % (H - h + 1), (g2 >> 32) % (W - w + 1), h, w, fl
    h, w = H, W
    if 4 * W < 3 * H:
        h = (4 * W) // 3
    elif 3 * W > 4 * H:
        w = (4 * H) // 3
    return (H - h) // 2, (W - w) // 2, h, w, fl


def _rrc_taps(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(i0, i1, l0, l1) of every output coordinate of an axis resampled from n_in to n_out:
    half-pixel centres in Q16, floored; the weights are exact float32."""
    o = np.arange(n_out, dtype=np.int64)
    p = np.maximum((((2 * o + 1) * n_in) << 15) // n_out - 32768, 0)
    i0 = p >> 16
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (p & 0xFFFF).astype(np.float32) * np.float32(2.0 ** -16)
    return i0, i1, np.float32(1.0) - l1, l1


def reference_transform_rrc(img: np.ndarray, index: int, epoch: int, seed: int, train: bool,
                            out_size: Sequence[int], flip: bool, mean, std) -> np.ndarray:
    """NumPy definition of the ``"rrc"`` per-sample transform (uint8 CHW -> float32 [C, Ho, Wo]):
    the :func:`reference_rrc_box` box resampled bilinearly to ``out_size``, flipped, normalised.
    The horizontal blend of 8-bit pixels with Q16 weights is exact in float32; the vertical one is
    two rounded multiplies and a rounded add; then ``v * scale + offset`` as in
    :func:`reference_transform`.  The native loader and the device kernel match it bit for bit."""
    C, H, W = img.shape
    Ho, Wo = (int(v) for v in out_size)
    _check_rrc_geometry(H, W, Ho, Wo)
    y0, x0, h, w, fl = reference_rrc_box(seed, epoch, index, H, W, train, flip)
    ry0, ry1, ly0, ly1 = _rrc_taps(h, Ho)
    cx0, cx1, lx0, lx1 = _rrc_taps(w, Wo)
    if fl:  # output column ox takes the taps of column Wo-1-ox
        cx0, cx1, lx0, lx1 = cx0[::-1], cx1[::-1], lx0[::-1], lx1[::-1]
    box = img[:, y0:y0 + h, x0:x0 + w].astype(np.float32)
    r0, r1 = box[:, ry0], box[:, ry1]
    top = r0[:, :, cx0] * lx0 + r0[:, :, cx1] * lx1
    bot = r1[:, :, cx0] * lx0 + r1[:, :, cx1] * lx1
    a = top * ly0[None, :, None]
    b = bot * ly1[None, :, None]
    v = a + b
    m = np.asarray(mean, np.float32)[:, None, None]
    s = np.asarray(std, np.float32)[:, None, None]
    return (v * (1.0 / (255.0 * s)) + (-m / s)).astype(np.float32)


# ------------------------------------------------------------------ per-sample augmentation
# TrivialAugmentWide on the stored uint8 image and Random Erasing on the normalised output
# (csrc/common/augment.hpp holds the native copy).  Integer arithmetic only: these functions are
# the contract the host loader and the device kernels (csrc/kernels/augment.hip) match byte for byte.
AUG_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness",
           "Color", "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
AUG_BINS = 31
AUG_POLICIES = ("ta_wide",)
_AUG_SALT = 0x5441776964654F70
_ERASE_SALT = 0x52616E6445726173
# round(65536 * cos / sin(4.5 deg * m)): Rotate's 31 angles
COS_Q16 = (65536, 65334, 64729, 63725, 62328, 60547, 58393, 55879, 53020, 49834, 46341, 42562,
           38521, 34242, 29753, 25080, 20252, 15299, 10252, 5142, 0, -5142, -10252, -15299,
           -20252, -25080, -29753, -34242, -38521, -42562, -46341)
SIN_Q16 = (0, 5142, 10252, 15299, 20252, 25080, 29753, 34242, 38521, 42562, 46341, 49834, 53020,
           55879, 58393, 60547, 62328, 63725, 64729, 65334, 65536, 65334, 64729, 63725, 62328,
           60547, 58393, 55879, 53020, 49834, 46341)
# round(65536 * 0.3 * 11 ** (t/63)): Random Erasing's aspect ratios h/w, log-uniform over [0.3, 3.3]
ERASE_RATIO_Q16 = (
    19661, 20424, 21216, 22039, 22894, 23782, 24705, 25663, 26659, 27693, 28767, 29884, 31043,
    32247, 33498, 34798, 36148, 37550, 39007, 40520, 42092, 43725, 45422, 47184, 49014, 50916,
    52891, 54943, 57075, 59289, 61589, 63978, 66460, 69039, 71717, 74499, 77390, 80392, 83511,
    86751, 90116, 93612, 97244, 101017, 104936, 109007, 113236, 117629, 122192, 126933, 131857,
    136972, 142286, 147806, 153541, 159497, 165685, 172113, 178790, 185726, 192932, 200417,
    208192, 216269)


def _sample_word(seed: int, epoch: int, index: int) -> int:
    """h0: the crop / flip word of sample ``index`` in ``epoch``."""
    return _splitmix64(seed ^ _splitmix64(((epoch * 0x100000001B3) & _MASK64) ^ (index & _MASK64)))


def augment_force(op, m: int, sign: int) -> int:
    """The ``force`` word that pins an op (name or number), a magnitude bin and a sign (+1 / -1)."""
    op = AUG_OPS.index(op) if isinstance(op, str) else int(op)
    if not (0 <= op < len(AUG_OPS) and 0 <= m < AUG_BINS and sign in (1, -1)):
        raise ValueError(f"bad augmentation op {(op, m, sign)}")
    return op | (m << 8) | ((1 if sign > 0 else 0) << 16)


def erase_pq(p: float) -> int:
    """Random Erasing's probability as the 24-bit threshold ``round(p * 2**24)``."""
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"random_erase must be a probability in [0, 1], got {p}")
    return int(round(float(p) * (1 << 24)))


def reference_augment_params(seed: int, epoch: int, index: int, force: int = -1
                             ) -> Tuple[int, int, int]:
    """(op, m, sign) of TrivialAugmentWide for a sample: one of the 14 :data:`AUG_OPS`, one of 31
    magnitude bins and a sign, from ``a = splitmix64(h0 ^ 0x5441776964654f70)``.  ``force`` >= 0
    pins them instead: ``op | m << 8 | (sign > 0) << 16``."""
    if force >= 0:
        op, m, s = force & 0xFF, (force >> 8) & 0xFF, (force >> 16) & 1
        if force >> 17 or op >= len(AUG_OPS) or m >= AUG_BINS:
            raise ValueError(f"bad force word {force:#x}")
        return op, m, (1 if s else -1)
    a = _splitmix64(_sample_word(seed, epoch, index) ^ _AUG_SALT)
    op = ((a & 0xFFFFFFFF) * len(AUG_OPS)) >> 32
    m = (((a >> 32) & 0xFFFFFF) * AUG_BINS) >> 24
    return op, m, (1 if (a >> 60) & 1 else -1)


def _aug_blend(d, v, fq: int) -> np.ndarray:
    return np.clip((d * (65536 - fq) + v * fq + 32768) >> 16, 0, 255)


def _aug_grey(v: np.ndarray) -> np.ndarray:
    if v.shape[0] == 1:
        return v[0]
    return (19595 * v[0] + 38470 * v[1] + 7471 * v[2] + 32768) >> 16


def reference_augment_op(img: np.ndarray, op: int, m: int, sign: int) -> np.ndarray:
    """One op of the table on a uint8 [C, H, W] image (C 1 or 3) -> uint8 [C, H, W]; the
    definitions: Q16 factors, floor (arithmetic) shifts on integers, fill 0."""
    C, H, W = img.shape
    if C not in (1, 3):
        raise ValueError(f"augmentation needs 1 or 3 channels, got {C}")
    name = AUG_OPS[op]
    v = img.astype(np.int64)
    q = (64881 * m) // 30
    fq = 65536 + sign * q
    if name == "Identity" or (name == "Color" and C == 1):
        out = v
    elif name == "Brightness":
        out = _aug_blend(0, v, fq)
    elif name == "Color":
        out = _aug_blend(_aug_grey(v)[None], v, fq)
    elif name == "Contrast":
        n = H * W
        mean = (2 * int(_aug_grey(v).sum()) + n) // (2 * n)
        out = _aug_blend(mean, v, fq)
    elif name == "Sharpness":
        s = v.copy()
        if H > 2 and W > 2:
            acc = sum(v[:, 1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
                      for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 4 * v[:, 1:-1, 1:-1]
            s[:, 1:-1, 1:-1] = (acc + 6) // 13
        out = _aug_blend(s, v, fq)
    elif name == "Posterize":
        bits = 8 - (2 * m + 5) // 10
        out = v & ((0xFF << (8 - bits)) & 0xFF)
    elif name == "Solarize":
        out = np.where(2 * v < 510 - 17 * m, v, 255 - v)
    elif name == "AutoContrast":
        out = v.copy()
        for c in range(C):
            lo, hi = int(v[c].min()), int(v[c].max())
            if hi > lo:
                out[c] = ((v[c] - lo) * 255) // (hi - lo)
    elif name == "Equalize":
        out = v.copy()
        for c in range(C):
            h = np.bincount(img[c].ravel(), minlength=256).astype(np.int64)
            nz = np.nonzero(h)[0]
            if len(nz) < 2:
                continue
            step = (int(h.sum()) - int(h[nz[-1]])) // 255
            if step == 0:
                continue
            cum = np.concatenate([[0], np.cumsum(h)[:-1]])
            out[c] = np.minimum(255, (step // 2 + cum) // step)[v[c]]
    else:  # the geometric ops: inverse nearest-neighbour map in doubled centred coordinates
        A = D = 65536
        B = Cc = tx = ty = 0
        if name == "ShearX":
            B = -sign * q
        elif name == "ShearY":
            Cc = -sign * q
        elif name == "TranslateX":
            tx = -sign * ((32 * m) // 30)
        elif name == "TranslateY":
            ty = -sign * ((32 * m) // 30)
        else:
            A = D = COS_Q16[m]
            B, Cc = sign * SIN_Q16[m], -sign * SIN_Q16[m]
        u = (2 * np.arange(W, dtype=np.int64) + 1 - W)[None, :]
        w = (2 * np.arange(H, dtype=np.int64) + 1 - H)[:, None]
        su = ((A * u + B * w) >> 16) + 2 * tx
        sv = ((Cc * u + D * w) >> 16) + 2 * ty
        xs, ys = (su + W) >> 1, (sv + H) >> 1
        ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
        out = np.where(ok[None], v[:, np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)], 0)
    return out.astype(np.uint8)


def reference_augment(img: np.ndarray, index: int, epoch: int, seed: int, force: int = -1
                      ) -> np.ndarray:
    """TrivialAugmentWide of the stored uint8 [C, H, W] image of sample ``index``: the op of
    :func:`reference_augment_params` applied by :func:`reference_augment_op`.  It runs before the
    crop / ``"rrc"`` transform, which then reads its output instead of the stored image."""
    return reference_augment_op(img, *reference_augment_params(seed, epoch, index, force))


def _erase_attempt(seed: int, epoch: int, index: int, pq: int, Ho: int, Wo: int
                   ) -> Tuple[int, int, int, int, int]:
    """(y0, x0, h, w, k): the erase box and the attempt that was accepted; k = -1 (and an empty
    box) when the sample is not erased, k = -2 when all ten attempts were rejected."""
    e = _splitmix64(_sample_word(seed, epoch, index) ^ _ERASE_SALT)
    if (e & 0xFFFFFF) >= pq:
        return 0, 0, 0, 0, -1
    for k in range(10):
        g = _splitmix64((e + k + 1) & _MASK64)
        sq = 1311 + (((21627 - 1311) * (g & 0xFFFFFF)) >> 24)  # scale in Q16 over [0.02, 0.33)
        area = (Ho * Wo * sq) >> 16
        r = ERASE_RATIO_Q16[(g >> 24) & 63]
        h = math.isqrt((area * r) >> 16)
        w = math.isqrt((area << 16) // r)
        if 0 < h < Ho and 0 < w < Wo:
            g2 = _splitmix64(g)
            return (g2 & 0xFFFFFFFF) % (Ho - h + 1), (g2 >> 32) % (Wo - w + 1), h, w, k
    return 0, 0, 0, 0, -2


def reference_erase_box(seed: int, epoch: int, index: int, pq: int, Ho: int, Wo: int
                        ) -> Optional[Tuple[int, int, int, int]]:
    """(y0, x0, h, w) of the Random Erasing box on the Ho x Wo output of a sample, or None: the
    sample is erased iff the low 24 bits of ``e = splitmix64(h0 ^ 0x52616e6445726173)`` are below
    ``pq`` = round(p * 2**24); torchvision's ``get_params`` (scale 0.02-0.33, log-uniform ratio
    0.3-3.3, ten attempts) in integers.  Every channel of the box becomes 0.0."""
    y0, x0, h, w, k = _erase_attempt(seed, epoch, index, pq, Ho, Wo)
    return (y0, x0, h, w) if k >= 0 else None


class RecordDataLoader:
    """Iterates (x [B,C,H,W] float32, y [B] int64) batches of this rank's shard.

    ``sampler`` follows :class:`DistributedSampler` semantics (``set_epoch`` reshuffles);
    batches land on ``device`` (pinned staging + non_blocking copy for GPU devices).

    ``decode="host"`` (default): the loader's CPU threads crop / flip / normalise and the float32
    batch is uploaded.  ``decode="device"``: the threads only gather the uint8 records (raw
    mode), the records and their sample indices are uploaded (a quarter of the bytes) and
    ``ops.kernels.record_decode`` runs the same transform on ``device`` — the same bits as the
    host path.  ``out_dtype``: dtype of ``x`` (float32 or bfloat16).  ``label_bytes``: width of
    the little-endian label in front of every record.

    ``transform="crop"`` (default) is RandomCrop(``pad``) + flip + Normalize at the stored size.
    ``transform="rrc"`` is :func:`reference_transform_rrc`: RandomResizedCrop + flip + Normalize
    in training, a 7/8 centre crop in evaluation, resized to ``out_size`` = (Ho, Wo) (default: the
    stored size); ``pad`` is not used.  Both work with either ``decode``.

    ``auto_augment="ta_wide"``: TrivialAugmentWide, one of 14 ops per image at one of 31
    magnitudes (:func:`reference_augment`).  ``random_erase=p``: Random Erasing with probability
    ``p`` (:func:`reference_erase_box`; scale 0.02-0.33, ratio 0.3-3.3, value 0.0).  The order is
    augment -> crop / rrc -> erase: the augmentation acts on the *stored* uint8 image, before the
    crop (torchvision augments the cropped image), so that the decode transforms and their
    bit-exact contracts stay as they are; the erase acts on the normalised output.  Both are
    integer-only functions of (seed, epoch, sample index), identical for ``decode="host"`` and
    ``decode="device"`` (csrc/kernels/augment.hip: ``record_augment`` before the decode kernel,
    ``batch_erase_`` after it).  ``train=False`` ignores both and launches nothing new."""

    def __init__(self, files: Sequence[str], shape: Sequence[int], batch_size: int,
                 sampler: Optional[DistributedSampler] = None, train: bool = True,
                 pad: int = 4, flip: bool = True, mean=CIFAR10_MEAN, std=CIFAR10_STD,
                 seed: int = 0, workers: int = 8, prefetch: int = 4, drop_last: bool = False,
                 device: Optional[torch.device] = None, decode: str = "host",
                 out_dtype: torch.dtype = torch.float32, label_bytes: int = 1,
                 transform: str = "crop", out_size: Optional[Sequence[int]] = None,
                 auto_augment: Optional[str] = None, random_erase: float = 0.0):
        from mipipe.runtime import runtime, runtime_available
        if decode not in ("host", "device"):
            raise ValueError(f"decode must be 'host' or 'device', got {decode!r}")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
        if transform not in ("crop", "rrc"):
            raise ValueError(f"transform must be 'crop' or 'rrc', got {transform!r}")
        if auto_augment in ("none", ""):
            auto_augment = None
        if auto_augment is not None and auto_augment not in AUG_POLICIES:
            raise ValueError(f"auto_augment must be None or one of {AUG_POLICIES}, "
                             f"got {auto_augment!r}")
        pq = erase_pq(random_erase)
        self.shape = tuple(int(v) for v in shape)
        if auto_augment is not None and self.shape[0] not in (1, 3):
            raise ValueError(f"auto_augment needs 1 or 3 channels, got {self.shape[0]}")
        # evaluation is never augmented and never erased
        self.auto_augment = auto_augment if train else None
        self.erase_pq = pq if train else 0
        self.transform = transform
        if transform == "crop":
            if out_size is not None and tuple(out_size) != self.shape[1:]:
                raise ValueError("out_size needs transform='rrc' (the crop transform keeps the "
                                 "stored size)")
            self.out_size = self.shape[1:]
        else:
            self.out_size = (tuple(int(v) for v in out_size) if out_size is not None
                             else self.shape[1:])
            if len(self.out_size) != 2:
                raise ValueError(f"out_size must be (Ho, Wo), got {out_size!r}")
            _check_rrc_geometry(*self.shape[1:], *self.out_size)
        self.batch_size = batch_size
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.train, self.pad, self.flip = train, pad, flip
        self.mean, self.std, self.seed = tuple(mean), tuple(std), seed
        self.decode, self.out_dtype = decode, out_dtype
        self.label_bytes = _check_label_bytes(label_bytes)
        self.epoch = 0
        self.files = list(files)
        self.native = runtime_available()
        C, H, W = self.shape
        self.record_bytes = self.label_bytes + C * H * W
        if self.native:
            cfg = runtime().LoaderConfig()
            cfg.files = self.files
            cfg.C, cfg.H, cfg.W = self.shape
            cfg.batch = batch_size
            cfg.label_bytes = self.label_bytes
            cfg.train, cfg.pad, cfg.flip = train, pad if train else 0, flip and train
            cfg.mean, cfg.std = list(map(float, mean)), list(map(float, std))
            cfg.seed, cfg.workers, cfg.prefetch, cfg.drop_last = seed, workers, prefetch, drop_last
            cfg.raw = decode == "device"
            if transform == "rrc":
                cfg.transform = "rrc"
                cfg.out_h, cfg.out_w = self.out_size
            if decode == "host":  # raw mode gathers only: the device augments and erases
                if self.auto_augment is not None:
                    cfg.auto_augment = self.auto_augment
                if self.erase_pq:
                    cfg.erase_pq = self.erase_pq
            self._ld = runtime().RecordLoader(cfg)
            n = len(self._ld)
        else:
            raws = [np.fromfile(f, dtype=np.uint8).reshape(-1, self.record_bytes)
                    for f in self.files]
            self._raw = (np.concatenate(raws) if raws
                         else np.zeros((0, self.record_bytes), np.uint8))
            self._imgs = self._raw[:, self.label_bytes:].reshape(-1, C, H, W)
            self._labels = _decode_labels(self._raw, self.label_bytes)
            n = len(self._labels)
        self.num_samples_total = n
        self.sampler = sampler if sampler is not None else DistributedSampler(n, shuffle=train,
                                                                               seed=seed)
        self.drop_last = drop_last
        pin = self.device.type == "cuda"
        if decode == "device":
            # the transform's constants, computed in float32 exactly as loader.cpp does
            m32, s32 = np.asarray(self.mean, np.float32), np.asarray(self.std, np.float32)
            affine = np.stack([np.float32(1.0) / (np.float32(255.0) * s32), -m32 / s32])
            self._affine = torch.from_numpy(affine.astype(np.float32)).to(self.device)
            self._stage = [(torch.empty(batch_size, self.record_bytes, dtype=torch.uint8,
                                        pin_memory=pin),
                            torch.empty(batch_size, dtype=torch.int64, pin_memory=pin))
                           for _ in range(2)]
        else:
            Ho, Wo = self.out_size
            self._stage = [(torch.empty(batch_size, C, Ho, Wo, dtype=torch.float32,
                                        pin_memory=pin),
                            torch.empty(batch_size, dtype=torch.int64, pin_memory=pin))
                           for _ in range(2)]

    def __len__(self) -> int:
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch
        self.sampler.set_epoch(epoch)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        self.epoch = getattr(self.sampler, "epoch", self.epoch)  # follow sampler.set_epoch
        idx = list(iter(self.sampler))
        if self.decode == "device":
            yield from self._iter_device(idx)
        elif self.native:
            self._ld.start_epoch(idx, self.epoch)
            k = 0
            events = [None, None]
            while True:
                xs, ys = self._stage[k % 2]
                if events[k % 2] is not None:
                    events[k % 2].synchronize()  # the H2D copy out of this staging buffer is done
                n = self._ld.next_into(xs.data_ptr(), ys.data_ptr())
                if n == 0:
                    return
                out = self._to_device(xs[:n], ys[:n])
                if self.device.type == "cuda":
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(self.device))
                    events[k % 2] = ev
                yield self._cast(out)
                k += 1
        else:
            for b in range(len(self)):
                sl = idx[b * self.batch_size:(b + 1) * self.batch_size]
                x = np.stack([self._reference(i) for i in sl])
                yield self._cast(self._to_device(torch.from_numpy(x),
                                                 torch.from_numpy(self._labels[sl])))

    def _reference(self, i: int) -> np.ndarray:
        """Sample ``i`` through the NumPy definition of the configured transform."""
        img = self._imgs[i]
        if self.auto_augment is not None:
            img = reference_augment(img, i, self.epoch, self.seed)
        if self.transform == "rrc":
            x = reference_transform_rrc(img, i, self.epoch, self.seed, self.train,
                                        self.out_size, self.flip and self.train, self.mean,
                                        self.std)
        else:
            x = reference_transform(img, i, self.epoch, self.seed, self.train,
                                    self.pad if self.train else 0, self.flip and self.train,
                                    self.mean, self.std)
        if self.erase_pq:
            box = reference_erase_box(self.seed, self.epoch, i, self.erase_pq, *x.shape[1:])
            if box is not None:
                y0, x0, h, w = box
                x[:, y0:y0 + h, x0:x0 + w] = 0.0
        return x

    def _iter_device(self, idx) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """decode="device": upload the uint8 records + sample indices, transform on the device."""
        from mipipe.ops import kernels as K
        epoch = self.epoch

        def decode(rec, gi):
            if self.auto_augment is not None:
                rec = K.record_augment(rec, gi, self.shape, self.seed, epoch, self.label_bytes)
            if self.transform == "rrc":
                out = K.record_decode_rrc(rec, gi, self._affine, self.shape, self.out_size,
                                          self.seed, epoch, self.flip and self.train, self.train,
                                          self.label_bytes, self.out_dtype)
            else:
                out = K.record_decode(rec, gi, self._affine, self.shape, self.seed, epoch,
                                      self.pad if self.train else 0, self.flip and self.train,
                                      self.train, self.label_bytes, self.out_dtype)
            if self.erase_pq:
                K.batch_erase_(out[0], gi, self.seed, epoch, self.erase_pq)
            return out

        if not self.native:
            for b in range(len(self)):
                sl = idx[b * self.batch_size:(b + 1) * self.batch_size]
                rec, gi = self._to_device(torch.from_numpy(self._raw[sl]),
                                          torch.tensor(sl, dtype=torch.int64))
                yield decode(rec, gi)
            return
        self._ld.start_epoch(idx, epoch)
        k = 0
        events = [None, None]
        while True:
            rs, gs = self._stage[k % 2]
            if events[k % 2] is not None:
                events[k % 2].synchronize()  # the H2D copies out of this staging pair are done
            n = self._ld.next_raw_into(rs.data_ptr(), gs.data_ptr())
            if n == 0:
                return
            rec, gi = self._to_device(rs[:n], gs[:n])
            if self.device.type == "cuda":
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                events[k % 2] = ev
            yield decode(rec, gi)
            k += 1

    def _cast(self, batch):
        x, y = batch
        return (x if x.dtype == self.out_dtype else x.to(self.out_dtype)), y

    def _to_device(self, x: torch.Tensor, y: torch.Tensor):
        if self.device.type == "cpu":
            return x.clone(), y.clone()
        return x.to(self.device, non_blocking=True), y.to(self.device, non_blocking=True)
