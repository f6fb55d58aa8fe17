"""The plan integer's codec (csrc/kernels/plan.hpp).

The header is host-only; tools/plan_dump.cpp is built here with the system C++ compiler and run
once.  The oracle is the dispatch's historical arithmetic written out below, not the header:

  conv fwd / inference fwd / fwd-style dgrad:  tile = p if p < 0 else p % 16,
                                               splits = 1 if p < 16 else p // 16
  wgrad / gemm / gemm_gelu:  [gemm, gemm_gelu only: p >= 4096 -> p = -1]
                             p < 0 -> (-1, -1, no ws); else ws = p & 1024, clear it,
                             tile = p % 16, splits = p // 16 if p // 16 > 0 else -1
  set_tune_entry accepts:    p == -1 or (p >= 0 and p % 16 < n_tiles)
"""
import glob
import json
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI, N_TILES = -1, 8191, 15
CONV_SPLITS = (1, 2, 3, 4, 6, 8)
GEMM_SP = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32)


def conv_oracle(p):
    return (p if p < 0 else p % 16, 1 if p < 16 else p // 16)


def gemm_oracle(p, legacy):
    if legacy and p >= 4096:
        p = -1
    if p < 0:
        return (-1, -1, 0)
    ws = 1 if p & 1024 else 0
    p &= ~1024
    return (p % 16, p // 16 if p // 16 > 0 else -1, ws)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """({p: the 11 columns after p}, {(tile, sp, ws): (conv encoding, gemm encoding)})"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "a system C++ compiler is needed to build the plan dump"
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror",
                    "-I" + os.path.join(REPO, "csrc", "kernels"),
                    os.path.join(REPO, "tools", "plan_dump.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe, str(LO), str(HI), str(N_TILES)], stdout=subprocess.PIPE, check=True,
                       timeout=120, text=True)
    dec, enc = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "E":
            t, sp, ws, ec, eg = map(int, f[1:])
            enc[(t, sp, ws)] = (ec, eg)
        else:
            v = list(map(int, f))
            dec[v[0]] = tuple(v[1:])
    assert sorted(dec) == list(range(LO, HI + 1))
    return dec, enc


def test_decoders_match_the_historical_arithmetic(dump):
    dec, _ = dump
    for p in range(LO, HI + 1):
        d = dec[p]
        assert d[0:2] == conv_oracle(p), p
        assert d[2:5] == gemm_oracle(p, False), p
        assert d[5:8] == gemm_oracle(p, True), p
        assert d[8] == int(p == -1 or (p >= 0 and p % 16 < N_TILES)), p


def test_conv_round_trip(dump):
    dec, enc = dump
    for t in range(N_TILES):
        for sp in CONV_SPLITS:
            p = t if sp == 1 else t + 16 * sp  # splits 1 is the bare tile
            assert enc[(t, sp, 0)][0] == p
            assert dec[p][0:2] == (t, sp)
            assert dec[p][9] == p  # encode(decode(p))


def test_gemm_round_trip(dump):
    dec, enc = dump
    for t in range(N_TILES):
        for sp in GEMM_SP:
            for ws in (0, 1):
                p = (t + 16 * sp) | (1024 if ws else 0)
                assert enc[(t, sp, ws)][1] == p
                assert dec[p][2:5] == (t, sp if sp > 0 else -1, ws)
                assert dec[p][5:8] == dec[p][2:5]  # below 4096 the legacy rule changes nothing
                assert dec[p][10] == p  # encode(decode(p))


def test_shipped_tables_decode_to_plans_the_tuner_emits(dump):
    """Every shipped table value decodes, under its key's op, to a tile config that exists and
    a split count the op's candidate generator can produce (bindings.cpp)."""
    dec, _ = dump
    files = sorted(glob.glob(os.path.join(REPO, "mipipe", "ops", "tune_tables", "*.json")))
    assert files
    n = 0
    for path in files:
        with open(path) as fh:
            table = json.load(fh)
        for key, p in table.items():
            op = key.split("|")[0]
            where = (os.path.basename(path), key, p)
            assert LO <= p <= HI, where
            if op in ("fwd", "fwdbn", "fwdinf", "fwdinfr", "dgrad"):
                tile, splits = dec[p][0:2]
                assert splits in CONV_SPLITS, where
            elif op in ("wgrad", "wgradbn"):
                tile, splits, ws = dec[p][2:5]
                assert splits in ((4, 6, 8, 12, 16, 24, 32) if ws else (-1, 1, 2, 3, 4, 6, 8, 12, 16)), where
            else:
                assert op == "gemm", where
                tile, splits, ws = dec[p][5:8]
                assert splits in ((2, 3, 4, 6, 8) if ws else (-1, 1, 2, 4)), where
            assert 0 <= tile < N_TILES, where
            n += 1
    assert n > 0
