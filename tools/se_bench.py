"""The squeeze-excitation kernels (se.hip) alone at the six SE shapes of mobilenet_v3_large, b256,
224^2, bf16, against the composition of the kernels the tree had before them.

    se_fwd/hip           bn_act_pool_fwd (BatchNorm apply + activation + pool) + se_scale_fwd
    se_fwd/composition   affine_act (ReLU) or affine_act + ATen hardswish, global_avg_pool
                         (avgpool_fwd), ATen hardsigmoid and a broadcast multiply
    se_bwd/hip           se_scale_bwd + bn_act_pool_bwd_reduce + bn_act_pool_bwd_apply
    se_bwd/composition   the multiply's two gradients, avgpool_bwd and an add, ATen hardswish
                         backward, bn_generic_bwd_reduce + bn_generic_bwd_apply

After the depthwise conv the shapes are 28^2 x 72 and 28^2 x 120 (ReLU rows), 14^2 x 480,
14^2 x 672, 7^2 x 672 and 7^2 x 960 (Hardswish rows).  The two FCs between pool and gate are the
same in both candidates and are left out.  All candidates run in ONE process on the same buffers,
alternated ``--reps`` times (at least four); a timed loop is ``--iters`` calls between two device
events after ``--warmup`` untimed calls, and the shader clock is sampled meanwhile
(mipipe/obs/clocks.py).  ``bytes_min`` counts every activation-sized tensor the fused form must
read or write once.  Back-to-back calls on these working sets (up to 58 MB) read partly from the
memory-side cache: an upper bound for a training step.

``--resources`` instead compiles se.hip for the device and prints the compiler's VGPR / LDS /
scratch figures per kernel instantiation (needs hipcc, no GPU).

Usage: python tools/se_bench.py [--batch 256] [--reps 4] [--iters 10] [--out FILE]
       python tools/se_bench.py --resources [--out FILE]
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

SHAPES = [(28, 72, "relu"), (28, 120, "relu"), (14, 480, "hardswish"), (14, 672, "hardswish"),
          (7, 672, "hardswish"), (7, 960, "hardswish")]


def resource_usage():
    """[{kernel, vgprs, lds_bytes, scratch_bytes, occupancy}] of se.hip for gfx950."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    arch = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(
            [hipcc, "-O3", "-std=c++17", f"-I{os.path.join(REPO, 'csrc')}", "-DNDEBUG",
             f"--offload-arch={arch}", "-munsafe-fp-atomics", "--cuda-device-only", "-c",
             os.path.join(REPO, "csrc", "kernels", "se.hip"), "-o", os.path.join(tmp, "se.o"),
             "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    out, cur = [], None
    keys = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes",
            "LDS Size [bytes/block]": "lds_bytes", "Occupancy [waves/SIMD]": "occupancy"}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN6mipipe12_GLOBAL__N_1\d+", "", m.group(1))
            name = re.sub(r"EEvPK.*|EPKf.*", "", name).replace("IDF16b", "<bf16").replace("If", "<fp32")
            name = name.replace("Li1E", ",relu").replace("Li3E", ",hardswish")
            name = name.replace("Lb1E", ",1").replace("Lb0E", ",0")
            cur = {"kernel": name + (">" if "<" in name else "")}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=256)
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
    import torch.nn.functional as F
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("se_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"se_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    bf = torch.bfloat16
    B = a.batch
    with ClockSampler(0) as cs:
        for hw, C, act in SHAPES:
            torch.manual_seed(0)
            y = torch.randn(B, hw, hw, C, device="cuda").to(bf)
            dout = torch.randn(B, hw, hw, C, device="cuda").to(bf)
            gate = torch.randn(B, C, device="cuda").to(bf)
            dpm = torch.randn(B, C, device="cuda")
            scale, bias = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
            mean, invstd = torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5
            gamma = torch.rand(C, device="cuda") + 0.5
            count = B * hw * hw
            z = K.bn_act_pool_fwd(y, scale, bias, act, False)[0]
            u = K.affine_act(y, scale, bias, "none")

            def hip_fwd():
                zz, pm = K.bn_act_pool_fwd(y, scale, bias, act, True)
                return K.se_scale_fwd(zz, gate), pm

            def comp_fwd():
                if act == "relu":
                    zz = K.affine_act(y, scale, bias, "relu")
                else:
                    zz = F.hardswish(K.affine_act(y, scale, bias, "none"))
                pm = K.avgpool_fwd(zz)
                return zz * F.hardsigmoid(gate).reshape(B, 1, 1, C), pm

            def hip_bwd():
                dz, dgate = K.se_scale_bwd(dout, z, gate)
                sg, sgx = K.bn_act_pool_bwd_reduce(dz, y, scale, bias, mean, invstd, act, dpm)
                return K.bn_act_pool_bwd_apply(dz, y, scale, bias, mean, invstd, gamma, act, dpm,
                                               sg, sgx), dgate

            def comp_bwd():
                s = F.hardsigmoid(gate)
                dz = dout * s.reshape(B, 1, 1, C)
                dgate = (dout.float() * z.float()).sum((1, 2)) * ((gate > -3) & (gate < 3)) / 6
                dz = dz + K.avgpool_bwd(dpm.to(bf), z.shape)
                if act == "relu":
                    sg, sgx = K.bn_generic_bwd_reduce(dz, z, y, mean, invstd, "relu")
                    return K.bn_generic_bwd_apply(dz, z, y, mean, invstd, gamma, sg, sgx, count,
                                                  "relu"), dgate
                du = torch.ops.aten.hardswish_backward(dz, u)
                sg, sgx = K.bn_generic_bwd_reduce(du, None, y, mean, invstd, "none")
                return K.bn_generic_bwd_apply(du, None, y, mean, invstd, gamma, sg, sgx, count,
                                              "none"), dgate

            elems = y.numel() * 2
            cands = {"se_fwd/hip": (hip_fwd, 4 * elems), "se_fwd/composition": (comp_fwd, 4 * elems),
                     "se_bwd/hip": (hip_bwd, 8 * elems), "se_bwd/composition": (comp_bwd, 8 * elems)}
            for fn, _ in cands.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            us = {k: [] for k in cands}
            for _ in range(a.reps):
                for k, (fn, _) in cands.items():
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
                    rec = {"shape": [B, hw, hw, C], "act": act, "candidate": name,
                           "us_per_call": round(med, 2), "us_all": [round(v, 2) for v in us[name]],
                           "bytes_min": cands[name][1],
                           "TB_per_s": round(cands[name][1] / med / 1e6, 3)}
                    if name == k:
                        rec["vs"] = ref
                        rec["speedup"] = round(statistics.median(us[ref]) / med, 3)
                        rec["faster_in_every_alternation"] = all(
                            h < r for h, r in zip(us[k], us[ref]))
                    emit(rec)
    emit({"batch": B, "dtype": "bf16", "gpu_clocks": cs.summary(), "reps": a.reps,
          "iters": a.iters})
    return finish()


if __name__ == "__main__":
    sys.exit(main())
