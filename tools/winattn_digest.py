"""Bit digests of the window-attention kernels (csrc/kernels/winattn.hip, winattn8.hip) and
patch_merge.

The contracts of these kernels against ``mipipe.ops._ref`` are tolerances, so a refactor that
must keep every bit is checked against the build it refactors instead: run this file on both
builds and compare the outputs line by line (the kernels repeat bit for bit, so a differing line
is a change).  Inputs come from CPU generators with fixed seeds; only ``native()`` entry points
are called.  The attention cases are the shapes of ``CASES`` in tests/test_swin_kernels_gpu.py and
tests/test_swin_v2_kernels_gpu.py (every mask region, the wrapped border on one axis only, the
partial last group and the grid stride), each with fresh gradient targets and with accumulators
pre-filled with 2.0.  Prints

    <case> <sha256 over the case's output buffers>

Usage: python tools/winattn_digest.py [--out FILE]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.flat_kernels_digest import digest  # noqa: E402

D = 32
LOGIT_SCALES = (math.log(10.0), math.log(200.0), -1.0)  # the second is clamped at ln 100


def cases(win, run, max_runs):
    """{name: (B, Hs, Ws, H, sy, sx)} for win x win windows, shift s = win // 2."""
    w, s = win, win // 2
    return {"one_window": (1, w, w, 1, 0, 0), "all_regions": (2, 2 * w, 2 * w, 3, s, s),
            "non_square": (1, 2 * w, 3 * w, 2, s, s), "single_window_axis": (1, w, 2 * w, 2, 0, s),
            "past_caps": (run * max_runs + run + 1, w, w, 1, s if win == 7 else 0,
                          s if win == 7 else 0)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)

    import torch
    from mipipe.ops._native import load_error, native, native_available

    if not torch.cuda.is_available():
        print("winattn_digest: no GPU", file=sys.stderr)
        return 2
    if not native_available():
        print(f"winattn_digest: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2
    C = native()
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    lines = []

    def emit(case, *tensors):
        torch.cuda.synchronize()
        s = f"{case} {digest(*tensors)}"
        print(s, flush=True)
        lines.append(s)

    def inputs(shape):
        B, Hs, Ws, H, _, _ = shape
        g = torch.Generator().manual_seed(Hs * 100 + Ws * 10 + H)
        T = B * Hs * Ws
        qkv = (torch.randn(T, 3 * H * D, generator=g) * 1.5).to(bf).to(dev)
        do = torch.randn(T, H * D, generator=g).to(bf).to(dev)
        return g, qkv, do

    for name, shape in cases(7, C.WIN_RUN, C.WIN_MAX_RUNS).items():
        H = shape[3]
        g, qkv, do = inputs(shape)
        table = (torch.randn(169, H, generator=g) * 0.5).to(dev).reshape(-1)
        emit(f"v1/{name}/o", C.winattn_fwd(qkv, table, *shape))
        dqkv, dtable = C.winattn_bwd(do, qkv, table, *shape)
        emit(f"v1/{name}/fresh/dqkv", dqkv)
        emit(f"v1/{name}/fresh/dtable", dtable)
        acc = torch.full((169 * H,), 2.0, device=dev)
        dqkv, none = C.winattn_bwd(do, qkv, table, *shape, dtable=acc)
        emit(f"v1/{name}/acc/dqkv", dqkv, none)
        emit(f"v1/{name}/acc/dtable", acc)

    for name, shape in cases(8, C.WIN8_RUN, C.WIN8_MAX_RUNS).items():
        H = shape[3]
        g, qkv, do = inputs(shape)
        bias = (16 * torch.sigmoid(torch.randn(225, H, generator=g))).to(dev)
        ls = torch.tensor([LOGIT_SCALES[i % 3] for i in range(H)]).to(dev)
        emit(f"v2/{name}/o", C.winattn8_fwd(qkv, bias, ls, *shape))
        dqkv, dbias, dls = C.winattn8_bwd(do, qkv, bias, ls, *shape)
        emit(f"v2/{name}/fresh/dqkv", dqkv)
        emit(f"v2/{name}/fresh/dbias", dbias)
        emit(f"v2/{name}/fresh/dlogit_scale", dls)
        accb = torch.full((225 * H,), 2.0, device=dev)
        accl = torch.full((H,), 2.0, device=dev)
        dqkv, nb, nl = C.winattn8_bwd(do, qkv, bias, ls, *shape, dbias=accb, dlogit_scale=accl)
        emit(f"v2/{name}/acc/dqkv", dqkv, nb, nl)
        emit(f"v2/{name}/acc/dbias", accb)
        emit(f"v2/{name}/acc/dlogit_scale", accl)

    B, Hs, Ws, Cc = 3, 6, 10, 136
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B * Hs * Ws, Cc, generator=g).to(bf).to(dev)
    dy = torch.randn(B * Hs * Ws // 4, 4 * Cc, generator=g).to(bf).to(dev)
    emit("patch_merge/fwd", C.patch_merge(x, B, Hs, Ws, False))
    emit("patch_merge/bwd", C.patch_merge(dy, B, Hs, Ws, True))

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
