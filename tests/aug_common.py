"""Record sets and references shared by test_record_augment_cpu.py and test_record_augment_gpu.py."""
import functools

import numpy as np

from mipipe.data import records as R

SEED = 1234
PQ_HALF = 1 << 23  # random_erase = 0.5
MEANS = {1: R.MNIST_MEAN, 3: R.IMAGENET_MEAN}
STDS = {1: R.MNIST_STD, 3: R.IMAGENET_STD}
# (stored shape, label bytes, n, batch): record strides 3073, 785, 1175 (odd extents and an odd
# stride), 4802 (2 label bytes) and 13 (no interior pixel)
SHAPES = [((3, 32, 32), 1, 20, 7), ((1, 28, 28), 1, 20, 7), ((3, 17, 23), 2, 20, 7),
          ((3, 40, 40), 2, 20, 7), ((3, 2, 2), 1, 20, 7)]
SHAPE_IDS = ["3x32x32", "1x28x28", "3x17x23-lb2", "3x40x40-lb2", "3x2x2"]
# the random policy and the erase run over 64 samples
N_RANDOM = 64
RANDOM_SETS = [(s[0], s[1]) for s in SHAPES[:3]]
ERASE_OUTS = [(32, 32), (5, 7), (3, 40)]
MAGNITUDES = (0, 1, 15, 30)


@functools.lru_cache(maxsize=None)
def dataset(shape, n, label_bytes=1):
    """(records uint8 [n, rec_bytes], images, labels, global indices).  The images mix full-range
    noise, a narrow range and a few levels (so AutoContrast / Equalize take every branch, the
    constant image included); the indices are 7i + 3 shuffled, one of them beyond 2**32."""
    rng = np.random.default_rng(sum(shape) + n + label_bytes)
    C = shape[0]
    img = rng.integers(0, 256, size=(n, *shape), dtype=np.uint8)
    for i in range(n):
        if i % 4 == 1:
            img[i] = rng.integers(60, 140, size=shape, dtype=np.uint8)
        elif i % 4 == 2:
            img[i] = (rng.integers(0, 8, size=shape) * rng.integers(0, 30, size=(C, 1, 1))
                      + rng.integers(0, 40, size=(C, 1, 1))).clip(0, 255).astype(np.uint8)
        elif i % 8 == 3:
            img[i] = np.uint8(rng.integers(0, 256))
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
def forced_reference(shape, n, label_bytes, op, m, sign):
    """reference_augment_op of every image of the set with the op pinned (read-only)."""
    _, img, _, _ = dataset(shape, n, label_bytes)
    ref = np.stack([R.reference_augment_op(img[i], op, m, sign) for i in range(n)])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def random_reference(shape, n, label_bytes, epoch):
    """reference_augment of the set under the random policy (read-only)."""
    _, img, _, gidx = dataset(shape, n, label_bytes)
    ref = np.stack([R.reference_augment(img[i], int(gidx[i]), epoch, SEED) for i in range(n)])
    ref.setflags(write=False)
    return ref


def policy_draws(shape, n, label_bytes=1, epochs=(0, 1)):
    """(op, m, sign) of every sample and epoch of the set."""
    _, _, _, gidx = dataset(shape, n, label_bytes)
    return [R.reference_augment_params(SEED, e, int(gi)) for e in epochs for gi in gidx.tolist()]


def erase_draws(shape, n, out, pq, epochs=(0, 1)):
    """(y0, x0, h, w, k) of every sample and epoch: k the accepted attempt, -1 not applied, -2 all
    ten attempts rejected."""
    _, _, _, gidx = dataset(shape, n)
    return [R._erase_attempt(SEED, e, int(gi), pq, *out) for e in epochs for gi in gidx.tolist()]


def assert_policy_coverage(draws):
    assert {d[0] for d in draws} == set(range(len(R.AUG_OPS))), "every op"
    assert {d[2] for d in draws} == {1, -1}, "both signs"
    ms = {d[1] for d in draws}
    assert 0 in ms and 30 in ms and ms <= set(range(31)), "the end bins"


def assert_erase_coverage(draws_by_out):
    """Over the output sizes together: skipped, accepted at once, accepted after a rejection, all
    ten rejected, a box touching an edge; every box lies inside its output."""
    ks = set()
    edge = False
    for (Ho, Wo), draws in draws_by_out.items():
        for y0, x0, h, w, k in draws:
            ks.add(-1 if k == -1 else -2 if k == -2 else min(k, 1))
            if k >= 0:
                assert 0 < h < Ho and 0 < w < Wo and 0 <= y0 <= Ho - h and 0 <= x0 <= Wo - w
                edge |= y0 == 0 or x0 == 0 or y0 + h == Ho or x0 + w == Wo
    assert ks == {-1, -2, 0, 1}, ks
    assert edge, "a box touching an edge"


def erase_reference(x, gidx, epoch, pq):
    """x [n, C, Ho, Wo] (a NumPy array of any word type) with every sample's box zeroed."""
    out = x.copy()
    for s, gi in enumerate(gidx.tolist()):
        box = R.reference_erase_box(SEED, epoch, int(gi), pq, *x.shape[2:])
        if box is not None:
            y0, x0, h, w = box
            out[s, :, y0:y0 + h, x0:x0 + w] = 0
    return out


def transform_reference(img, gi, epoch, shape, transform, out, auto_augment, pq, pad=4):
    """One sample through augment -> crop / rrc -> erase, all NumPy."""
    C = shape[0]
    if auto_augment:
        img = R.reference_augment(img, gi, epoch, SEED)
    if transform == "rrc":
        x = R.reference_transform_rrc(img, gi, epoch, SEED, True, out, True, MEANS[C], STDS[C])
    else:
        x = R.reference_transform(img, gi, epoch, SEED, True, pad, True, MEANS[C], STDS[C])
    box = R.reference_erase_box(SEED, epoch, gi, pq, *x.shape[1:]) if pq else None
    if box is not None:
        y0, x0, h, w = box
        x[:, y0:y0 + h, x0:x0 + w] = 0.0
    return x
