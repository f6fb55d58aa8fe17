"""The depthwise kernels of dwconvk.hip alone at EfficientNet's shapes, bf16, timed in alternation
against the route the zoo used before them (rocprofv3 is not involved: HIP events around loops):

    fwd     K.dwconvk_fwd with the BatchNorm statistics   vs  K.gconv_fwd + K.chan_stats
    dgrad   K.dwconvk_dgrad                               vs  K.gconv_dgrad
    wgrad   K.dwconvk_wgrad into a pre-allocated target   vs  K.gconv_wgrad into the same

at b0's twelve depthwise shapes at 224 x 224 plus b4's largest and smallest (380 x 380).  One
JSON line per (shape, pass, candidate); ``faster_in_every_alternation`` is the rule the model's
route table (mipipe.models._zoo.DWCONVK_OLD_ROUTE) follows.  Back-to-back calls on these working
sets read partly from the memory-side cache: an upper bound for a training step.

``--resources`` instead compiles dwconvk.hip for the device and prints the compiler's VGPR /
scratch / occupancy figures per kernel instantiation with the LDS bytes it is launched with
(needs hipcc and the built extension, no GPU).

Usage: python tools/efficientnet_bench.py [--batch 64] [--reps 4] [--iters 10] [--out FILE]
       python tools/efficientnet_bench.py --resources [--out FILE]
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

#: (input rows, channels, kernel, stride): b0 at 224, then b4 at 380 (largest, smallest map)
SHAPES = [(112, 32, 3, 1), (112, 96, 3, 2), (56, 144, 3, 1), (56, 144, 5, 2), (28, 240, 5, 1),
          (28, 240, 3, 2), (14, 480, 3, 1), (14, 480, 5, 1), (14, 672, 5, 1), (14, 672, 5, 2),
          (7, 1152, 5, 1), (7, 1152, 3, 1), (190, 48, 3, 1), (12, 2688, 3, 1)]
LDS_PER_CU = 160 * 1024  # gfx950


def resource_usage():
    """[{kernel, vgprs, agprs, scratch_bytes, occupancy, lds_bytes, blocks_per_cu}] of dwconvk.hip
    for gfx950.  LDS is dynamic, so ``lds_bytes`` is the launcher's size (dwk_lds_bytes)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    arch = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(
            [hipcc, "-O3", "-std=c++17", f"-I{os.path.join(REPO, 'csrc')}", "-DNDEBUG",
             f"--offload-arch={arch}", "-munsafe-fp-atomics", "--cuda-device-only", "-c",
             os.path.join(REPO, "csrc", "kernels", "dwconvk.hip"), "-o", os.path.join(tmp, "k.o"),
             "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    out, cur = [], None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes",
            "LDS Size [bytes/block]": "lds_bytes", "Occupancy [waves/SIMD]": "occupancy"}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN6mipipe12_GLOBAL__N_1\d+", "", m.group(1))
            name = re.sub(r"EEvPK.*", "", name).replace("IDF16b", "<bf16").replace("If", "<fp32")
            name = re.sub(r"Li(\d)E", r",\1", name).replace("Lb1E", ",1").replace("Lb0E", ",0")
            cur = {"kernel": name + (">" if "<" in name else "")}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    from mipipe.ops._native import native
    for rec in out:  # the compiler sees 0 static bytes: the launch size of this instantiation
        m = re.match(r"dwconvk_(fwd|dgrad|wgrad)_kernel<\w+,(\d),(\d)", rec["kernel"])
        rec["lds_bytes"] = native().dwk_lds_bytes(m.group(1), int(m.group(2)), int(m.group(3)))
        # a block is 4 waves, one per SIMD: registers allow ``occupancy`` blocks on a CU
        rec["blocks_per_cu"] = min(rec["occupancy"], LDS_PER_CU // rec["lds_bytes"])
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=10, help="calls per timed loop")
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
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("efficientnet_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"efficientnet_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    bf = torch.bfloat16
    B = a.batch
    with ClockSampler(0) as cs:
        for hw, C, k, s in SHAPES:
            torch.manual_seed(0)
            p = (k - 1) // 2
            x = torch.randn(B, hw, hw, C, device="cuda").to(bf)
            w = torch.randn(C, k, k, 1, device="cuda").to(bf)
            shift = torch.randn(C, device="cuda")
            y = K.dwconvk_fwd(x, w, s)[0]
            dy = torch.randn(y.shape, device="cuda").to(bf)
            dw = torch.zeros(C, 1, k, k, device="cuda")
            dw_old = dw.permute(0, 2, 3, 1)
            st, pd = (s, s), (p, p)

            def old_fwd():
                yy = K.gconv_fwd(x, w, st, pd, C)
                return yy, K.chan_stats(yy, shift)

            cands = {
                "fwd/dwconvk": lambda: K.dwconvk_fwd(x, w, s, shift),
                "fwd/gconv+chan_stats": old_fwd,
                "dgrad/dwconvk": lambda: K.dwconvk_dgrad(dy, w, x.shape, s),
                "dgrad/gconv": lambda: K.gconv_dgrad(dy, w, x.shape, st, pd, C),
                "wgrad/dwconvk": lambda: K.dwconvk_wgrad(dy, x, k, s, dw.reshape(-1)),
                "wgrad/gconv": lambda: K.gconv_wgrad(dy, x, k, k, st, pd, C, out=dw_old)}
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
                    rec = {"shape": [B, hw, hw, C], "k": k, "stride": s, "candidate": name,
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
