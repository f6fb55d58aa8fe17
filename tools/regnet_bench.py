"""The grouped 3x3 kernels of gconv3.hip alone at RegNet's ``f.b`` shapes, bf16, timed in
alternation against the route ``XConv2d.run`` takes for the same conv (block_group_conv2d where
the group width divides 64, else the direct gconv kernels) plus ``chan_stats`` (HIP events around
loops, no profiler):

    fwd   MF.gconv3 with the BatchNorm statistics      vs  conv.run + K.chan_stats
    bwd   its backward (data-grad + weight-grad)       vs  conv.run's backward

at the f.b shapes of regnet_y_400mf, y_800mf, y_1_6gf, y_8gf and x_3_2gf at 224 x 224.  (The old
route's data-grad and weight-grad are not separate entries, so the backward is timed as one.)  One
JSON line per (shape, pass, candidate); ``faster_in_every_alternation`` is the rule the model's
route table (mipipe.models._zoo.GCONV3_OLD_ROUTE) follows.  Back-to-back calls on these working
sets read partly from the memory-side cache: an upper bound for a training step.

``--resources`` instead compiles gconv3.hip for the device and prints the compiler's VGPR / AGPR /
LDS / scratch / occupancy figures per kernel instantiation (needs hipcc, no GPU).

Usage: python tools/regnet_bench.py [--batch 64] [--reps 4] [--iters 5] [--out FILE]
       python tools/regnet_bench.py --resources [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MODELS = ("y_400mf", "y_800mf", "y_1_6gf", "y_8gf", "x_3_2gf")
LDS_PER_CU = 160 * 1024  # gfx950


def shapes():
    """Sorted distinct (group width, stride, channels, input rows) of the models' f.b convs."""
    from mipipe.models.regnet import _CONFIGS, stage_params
    out = set()
    for name in MODELS:
        depths, widths, groups = stage_params(*_CONFIGS[name])
        for i, (d, w, g) in enumerate(zip(depths, widths, groups)):
            out.add((g, 2, w, 112 >> i))
            if d > 1:
                out.add((g, 1, w, 56 >> i))
    return sorted(out)


def resource_usage():
    """[{kernel, vgprs, agprs, scratch_bytes, occupancy, lds_bytes, blocks_per_cu}] of gconv3.hip
    for gfx950 (LDS is static: the compiler's figure is the launch's)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    arch = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(
            [hipcc, "-O3", "-std=c++17", f"-I{os.path.join(REPO, 'csrc')}", "-DNDEBUG",
             f"--offload-arch={arch}", "-munsafe-fp-atomics", "--cuda-device-only", "-c",
             os.path.join(REPO, "csrc", "kernels", "gconv3.hip"), "-o", os.path.join(tmp, "k.o"),
             "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    out, cur = [], None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes",
            "LDS Size [bytes/block]": "lds_bytes", "Occupancy [waves/SIMD]": "occupancy"}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"(gconv3_\w+?_kernel)I((?:L[ib]\d+E)+)EEv", m.group(1))
            name = m.group(1) if k is None else \
                k.group(1) + "<" + ",".join(re.findall(r"L[ib](\d+)E", k.group(2))) + ">"
            cur = {"kernel": name}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    for rec in out:  # a block is 4 waves, one per SIMD: registers allow ``occupancy`` blocks on a CU
        rec["blocks_per_cu"] = min(rec["occupancy"], LDS_PER_CU // max(rec["lds_bytes"], 1))
    return sorted(out, key=lambda r: r["kernel"])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=5, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls per candidate")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 4)
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    def finish():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return 0

    if a.resources:
        for rec in resource_usage():
            emit(rec)
        return finish()

    import torch
    from mipipe import nn as mnn
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import functional as MF
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("regnet_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"regnet_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    bf = torch.bfloat16
    B = a.batch
    with ClockSampler(0) as cs:
        for G, s, C, hw in shapes():
            torch.manual_seed(0)
            conv = mnn.XConv2d(C, C, 3, s, 1, groups=C // G, bias=False).cuda()
            w_c = conv.compute_weight(bf)
            shift = torch.randn(C, device="cuda")
            x = torch.randn(B, hw, hw, C, device="cuda").to(bf).requires_grad_(True)
            dy = torch.randn_like(K.gconv3_fwd(x.detach(), w_c, s)[0])

            def new_fwd():
                return MF.gconv3(x, conv.weight, w_c, s, shift)[0]

            def old_fwd():
                y = conv.run(x)
                K.chan_stats(y.detach(), shift)
                return y

            def bwd(y):
                def run():
                    conv.weight.grad = None
                    torch.autograd.grad(y, (x, conv.weight), dy, retain_graph=True)
                return run

            cands = {"fwd/gconv3": new_fwd, "fwd/XConv2d.run+chan_stats": old_fwd,
                     "bwd/gconv3": bwd(new_fwd()), "bwd/XConv2d.run": bwd(conv.run(x))}
            for fn in cands.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name in cands}
            for _ in range(a.reps):
                for name, fn in cands.items():
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    us[name].append(e0.elapsed_time(e1) * 1e3 / a.iters)
            keys = list(cands)
            for i in range(0, len(keys), 2):
                new, old = keys[i], keys[i + 1]
                for name in (new, old):
                    rec = {"shape": [B, hw, hw, C], "G": G, "stride": s, "candidate": name,
                           "us_per_call": round(statistics.median(us[name]), 2),
                           "us_all": [round(v, 2) for v in us[name]]}
                    if name == new:
                        rec["vs"] = old
                        rec["speedup"] = round(statistics.median(us[old]) /
                                               statistics.median(us[new]), 3)
                        rec["faster_in_every_alternation"] = all(
                            h < r for h, r in zip(us[new], us[old]))
                    emit(rec)
    emit({"batch": B, "dtype": "bf16", "gpu_clocks": cs.summary(), "reps": a.reps,
          "iters": a.iters})
    return finish()


if __name__ == "__main__":
    sys.exit(main())
