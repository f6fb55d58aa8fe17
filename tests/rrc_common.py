"""Record sets and references shared by test_record_rrc_cpu.py and test_record_rrc_gpu.py."""
import functools

import numpy as np

from mipipe.data import records as R

SEED = 11
MEANS = {1: R.MNIST_MEAN, 3: R.IMAGENET_MEAN}
STDS = {1: R.MNIST_STD, 3: R.IMAGENET_STD}
# (stored shape, output size, n, batch)
CASES = [((3, 20, 24), (16, 16), 48, 5),    # box smaller / larger than the output, partial batch
         ((1, 9, 13), (7, 5), 48, 5),       # odd extents: the scalar store path
         ((3, 6, 300), (4, 260), 8, 3),     # every sample falls back; row wider than a block; 32x up
         ((3, 40, 40), (32, 32), 48, 16),
         ((3, 256, 256), (224, 224), 8, 8)]  # the workload's own geometry, once
IDS = ["3x20x24-16x16", "1x9x13-7x5", "3x6x300-4x260", "3x40x40-32x32", "3x256x256-224x224"]


@functools.lru_cache(maxsize=None)
def dataset(shape, n, label_bytes=1):
    """(records uint8 [n, rec_bytes], images, labels, global indices): the indices are 7i + 3
    shuffled, one of them moved beyond 2**32."""
    rng = np.random.default_rng(sum(shape) + n)
    img = rng.integers(0, 256, size=(n, *shape), dtype=np.uint8)
    lab = rng.integers(0, 256 if label_bytes < 2 else 1000, size=n).astype(np.int64)
    gidx = rng.permutation(7 * np.arange(n, dtype=np.int64) + 3)
    gidx[n // 2] += 1 << 40
    rec = np.empty((n, label_bytes + img[0].size), np.uint8)
    for k in range(label_bytes):
        rec[:, k] = (lab >> (8 * k)) & 0xFF
    rec[:, label_bytes:] = img.reshape(n, -1)
    for a in (rec, img, lab, gidx):
        a.setflags(write=False)
    return rec, img, lab, gidx


@functools.lru_cache(maxsize=None)
def reference(shape, out, n, train, epoch):
    """reference_transform_rrc of the whole set, computed once per case and shared (read-only)."""
    _, img, _, gidx = dataset(shape, n)
    C = shape[0]
    ref = np.stack([R.reference_transform_rrc(img[i], int(gidx[i]), epoch, SEED, train, out, train,
                                              MEANS[C], STDS[C]) for i in range(n)])
    ref.setflags(write=False)
    return ref


def boxes(shape, n, epochs=(0, 1)):
    """(y0, x0, h, w, flip, accepted attempt k or -1 for the fallback) of every sample and epoch."""
    _, _, _, gidx = dataset(shape, n)
    _, H, W = shape
    out = []
    for e in epochs:
        for gi in gidx.tolist():
            box = R.reference_rrc_box(SEED, e, gi, H, W, True)
            out.append(box + (_attempt(e, gi, H, W),))
    return out


def _attempt(epoch, gi, H, W):
    """Which attempt reference_rrc_box accepted, re-derived from the issue's definition."""
    import math
    h0 = R._splitmix64(SEED ^ R._splitmix64(((epoch * 0x100000001B3) & R._MASK64) ^ gi))
    for k in range(10):
        g = R._splitmix64((h0 + k + 1) & R._MASK64)
        area = (H * W * (5243 + (((65536 - 5243) * (g & 0xFFFFFF)) >> 24))) >> 16
        r = R.RATIO_Q16[(g >> 24) & 63]
        w, h = math.isqrt((area * r) >> 16), math.isqrt((area << 16) // r)
        if 0 < w <= W and 0 < h <= H:
            return k
    return -1
