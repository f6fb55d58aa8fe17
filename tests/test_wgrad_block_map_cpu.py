"""Placement of split-K weight-grad blocks (csrc/kernels/block_map.hpp splitk_block_map).

The helper is host + device code; its host side is built here with the system C++ compiler into
a small stand-alone program (tools/wgrad_block_map_dump.cpp) that dumps the map for every
(tiles, splits) in 1..72 x 1..72.  The hardware deals linear workgroup ids round-robin over the 8
XCDs: block L runs on XCD class L % 8, in dispatch slot L // 8 of that class.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMAX = SMAX = 72
NX = 8


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{(tiles, splits): (tile[L], split[L])} from one run of the dump program."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "a system C++ compiler is needed to build the block-map dump"
    exe = str(tmp_path_factory.mktemp("block_map") / "wgrad_block_map_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I" + os.path.join(REPO, "csrc", "kernels"),
                    os.path.join(REPO, "tools", "wgrad_block_map_dump.cpp"), "-o", exe],
                   check=True, timeout=120)
    r = subprocess.run([exe, str(TMAX), str(SMAX)], stdout=subprocess.PIPE, check=True, timeout=120)
    raw = np.frombuffer(r.stdout, dtype="<u2").astype(np.int64)
    out, off = {}, 0
    for tiles in range(1, TMAX + 1):
        for splits in range(1, SMAX + 1):
            n = tiles * splits
            pair = raw[off:off + 2 * n].reshape(n, 2)
            out[(tiles, splits)] = (pair[:, 0], pair[:, 1])
            off += 2 * n
    assert off == raw.size
    return out


def test_bijection(maps):
    """(a) every (tile, split) of tiles x splits is produced by exactly one block."""
    for (tiles, splits), (tile, split) in maps.items():
        n = tiles * splits
        assert tile.size == n
        assert (tile < tiles).all() and (split < splits).all(), (tiles, splits)
        assert np.array_equal(np.sort(split * tiles + tile), np.arange(n)), (tiles, splits)


def test_class_runs_consecutive_split_major(maps):
    """(b) for each XCD class L % 8 the mapped pairs, in slot order L // 8, are consecutive in
    split-major order (tile fastest): adjacent dispatch slots of an XCD run adjacent tiles of one
    k-slice and move to the next slice only at its end."""
    for (tiles, splits), (tile, split) in maps.items():
        v = split * tiles + tile
        for c in range(NX):
            run = v[c::NX]
            assert (np.diff(run) == 1).all(), (tiles, splits, c)


def test_split_spans_few_classes(maps):
    """(c) a k-slice's tiles fall into at most two XCD classes whenever every class can hold a
    whole slice (splits >= 8: each class owns >= tiles consecutive pairs).  With fewer than 8
    splits no bijective map can do that — a class has only tiles*splits/8 < tiles slots — so
    there the bound is what contiguous class runs of length >= q = (tiles*splits) // 8 allow:
    a slice of t >= 2 tiles touches at most 2 + (t - 2) // q runs.  Grids of fewer than 8 blocks
    are left as they are (every block its own XCD)."""
    for (tiles, splits), (tile, split) in maps.items():
        n = tiles * splits
        cls = np.arange(n) % NX
        for s in range(splits):
            k = np.unique(cls[split == s]).size
            if n < NX:
                assert k == tiles, (tiles, splits, s)
                continue
            q = n // NX
            bound = 1 if tiles == 1 else 2 + (tiles - 2) // q
            assert k <= bound, (tiles, splits, s, k)
            if splits >= NX:
                assert k <= 2, (tiles, splits, s, k)


def test_unsplit_is_the_tile_remap(maps):
    """splits == 1 is the plain XCD tile remap of the unsplit kernels (forward / data-grad)."""
    for tiles in range(1, TMAX + 1):
        tile, split = maps[(tiles, 1)]
        assert (split == 0).all()
        q, r = divmod(tiles, NX)
        for L in range(tiles):
            x, slot = L % NX, L // NX
            want = L if tiles < NX else (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + slot
            assert tile[L] == want, (tiles, L)
