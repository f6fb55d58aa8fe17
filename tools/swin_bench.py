"""The Swin kernels alone at the four stage shapes of swin_t, B = 64, bf16, against the ATen
composition that ``SwinTransformer.reference_forward`` uses, on the same tensors.

    window_attention fwd / fwd+bwd   hip (winattn.hip)  vs  aten: roll, window partition, two batched
                                                           matmuls, bias gather, mask, softmax,
                                                           reverse, un-roll (autograd backward)
    patch_merge fwd                  hip                vs  aten: four strided slices + cat

Maps 56^2 x 3 heads, 28^2 x 6, 14^2 x 12, 7^2 x 24, shift 0 and 3.  All candidates run in ONE
process on the same buffers, alternated ``--reps`` times (at least four); a timed loop is
``--iters`` calls between two device events after ``--warmup`` untimed calls, and the shader clock
is sampled meanwhile (mipipe/obs/clocks.py).  Per candidate: the µs per call of every alternation
and the median.  ``--resources`` instead compiles winattn.hip for the device and prints the
compiler's VGPR / LDS / scratch figures per kernel (no GPU needed).

``--v2`` measures Swin V2's cosine window attention (winattn8.hip) the same way at swin_v2_t's
stage shapes, maps 64^2 x 3 heads, 32^2 x 6, 16^2 x 12, 8^2 x 24, shift 0 and 4, against the ATen
composition of ``SwinTransformerV2.reference_forward`` (F.normalize, the temperature, the gathered
bias); the output then starts with winattn8.hip's resource figures.

Usage: python tools/swin_bench.py [--v2] [--batch 64] [--reps 4] [--iters 10]
                                  [--out profiles/swin_kernels.txt] | --resources
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

STAGES = [(56, 3), (28, 6), (14, 12), (7, 24)]
STAGES_V2 = [(64, 3), (32, 6), (16, 12), (8, 24)]


def resources(src="winattn.hip"):
    """[{kernel, vgprs, agprs, lds_bytes, scratch_bytes, occupancy}] of a kernel file for gfx950."""
    from tools.build_ext import ARCH, CSRC, HIPCC, _NO_PACKED_FP32
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(
            [HIPCC, "-O3", "-std=c++17", f"-I{CSRC}", "-DNDEBUG", f"--offload-arch={ARCH}",
             "-munsafe-fp-atomics", *_NO_PACKED_FP32, "-Rpass-analysis=kernel-resource-usage",
             "-c", os.path.join(CSRC, "kernels", src), "-o", os.path.join(tmp, "w.o")],
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    out, cur = [], None
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        key = {"Function Name": "kernel", "VGPRs": "vgprs", "AGPRs": "agprs",
               "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "occupancy",
               "LDS Size [bytes/block]": "lds_bytes"}[m.group(1)]
        if key == "kernel":
            cur = {"kernel": m.group(2)}
            out.append(cur)
        else:
            cur[key] = int(m.group(2))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=10, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls per candidate")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--v2", action="store_true", help="Swin V2: winattn8.hip, 8x8 windows")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 4)
    if a.resources:
        for rec in resources("winattn8.hip" if a.v2 else "winattn.hip"):
            print(json.dumps(rec))
        return 0

    import torch
    import torch.nn.functional as F
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import _ref
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("swin_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"swin_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    bf, B, lines = torch.bfloat16, a.batch, []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    W = 8 if a.v2 else 7  # window side
    N = W * W
    if a.v2:
        for rec in resources("winattn8.hip"):
            emit(rec)

    def aten_attention(qkv, table, rel, mask, hw, H, shift, ls=None):
        """reference_forward's attention on the packed projection, bf16 (``ls``: V2's logit
        scales — cosine scores times the clamped temperature instead of the scaled dot product)."""
        x = qkv.view(B, hw, hw, -1)
        if shift:
            x = torch.roll(x, (-shift, -shift), (1, 2))
        n, nW = hw // W, (hw // W) ** 2
        x = x.view(B, n, W, n, W, 3, H, 32).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * nW, H, N, 32)
        if ls is None:
            att = (x[0] * 32 ** -0.5) @ x[1].transpose(-2, -1)
        else:
            att = F.normalize(x[0], dim=-1) @ F.normalize(x[1], dim=-1).transpose(-2, -1)
            att = att * torch.clamp(ls, max=math.log(100.0)).exp().to(bf)
        att = att + table[rel].permute(2, 0, 1).to(bf)
        if shift:
            att = (att.view(B, nW, H, N, N) + mask[None, :, None]).view(B * nW, H, N, N)
        o = (F.softmax(att, -1) @ x[2]).view(B, n, n, H, W, W, 32).permute(0, 1, 4, 2, 5, 3, 6)
        o = o.reshape(B, hw, hw, H * 32)
        return (torch.roll(o, (shift, shift), (1, 2)) if shift else o).reshape(B * hw * hw, -1)

    with ClockSampler(0) as cs:
        for hw, H in (STAGES_V2 if a.v2 else STAGES):
            for shift in (0, W // 2):
                if shift and hw == W:
                    continue  # a single-window map is never shifted
                torch.manual_seed(0)
                T, C = B * hw * hw, H * 32
                qkv = torch.randn(T, 3 * C, device="cuda").to(bf)
                do = torch.randn(T, C, device="cuda").to(bf)
                _, rel, m = _ref.window_geometry(hw, hw, shift, "cuda", W)
                mask = (m * -100.0).to(bf)
                if a.v2:
                    table = 16 * torch.sigmoid(torch.randn(225, H, device="cuda"))
                    ls = torch.full((H, 1, 1), math.log(10.0), device="cuda")
                    dt, dl = torch.zeros(225, H, device="cuda"), torch.zeros(H, device="cuda")
                    qa, ta, la = (t.clone().requires_grad_() for t in (qkv, table, ls))

                    def aten_fb():
                        qa.grad = ta.grad = la.grad = None
                        aten_attention(qa, ta, rel, mask, hw, H, shift, la).backward(do)

                    def hip_f():
                        return K.window_attention_v2_fwd(qkv, table, ls, B, hw, hw, H, shift)

                    def hip_fb():
                        hip_f()
                        K.window_attention_v2_bwd(do, qkv, table, ls, B, hw, hw, H, shift, dt, dl)

                    def aten_f():
                        return aten_attention(qkv, table, rel, mask, hw, H, shift, ls)
                else:
                    table = torch.randn(169, H, device="cuda") * 0.1
                    dt = torch.zeros(169 * H, device="cuda")
                    qa, ta = qkv.clone().requires_grad_(), table.clone().requires_grad_()

                    def aten_fb():
                        qa.grad = ta.grad = None
                        aten_attention(qa, ta, rel, mask, hw, H, shift).backward(do)

                    def hip_f():
                        return K.window_attention_fwd(qkv, table, B, hw, hw, H, shift)

                    def hip_fb():
                        hip_f()
                        K.window_attention_bwd(do, qkv, table, B, hw, hw, H, shift, dt)

                    def aten_f():
                        return aten_attention(qkv, table, rel, mask, hw, H, shift)

                name = "winattn8" if a.v2 else "winattn"
                cands = {
                    f"{name}_fwd/hip": hip_f,
                    f"{name}_fwd/aten": aten_f,
                    f"{name}_fwd_bwd/hip": hip_fb,
                    f"{name}_fwd_bwd/aten": aten_fb,
                }
                if not a.v2 and not shift and hw > 7:
                    x = torch.randn(T, C, device="cuda").to(bf)
                    cands["patch_merge_fwd/hip"] = lambda: K.patch_merge(x, B, hw, hw)
                    cands["patch_merge_fwd/aten"] = lambda: _ref.patch_merge(x, B, hw, hw)
                for fn in cands.values():
                    for _ in range(a.warmup):
                        fn()
                torch.cuda.synchronize()
                us = {k: [] for k in cands}
                for _ in range(a.reps):
                    for k, fn in cands.items():
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.iters):
                            fn()
                        e1.record()
                        e1.synchronize()
                        us[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
                keys = list(cands)
                for i in range(0, len(keys), 2):
                    k, ref = keys[i], keys[i + 1]
                    for name in (k, ref):
                        med = statistics.median(us[name])
                        rec = {"shape": [B, hw, hw, H], "shift": shift, "candidate": name,
                               "us_per_call": round(med, 2),
                               "us_all": [round(v, 2) for v in us[name]]}
                        if name == k:
                            rec["vs"] = ref
                            rec["speedup"] = round(statistics.median(us[ref]) / med, 3)
                            rec["faster_in_every_alternation"] = all(
                                h < r for h, r in zip(us[k], us[ref]))
                        emit(rec)
    emit({"batch": B, "dtype": "bf16", "gpu_clocks": cs.summary(), "reps": a.reps,
          "iters": a.iters})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
