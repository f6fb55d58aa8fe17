"""The Vision Transformer kernels alone at the vit_b_16 b256 shapes, against the ATen compositions.

``[256, 3, 224, 224]`` images with patch 16 and the ``[50432, 768]`` token stream (256 x 197):

    patchify        hip (fp32 image -> bf16 rows)   vs  aten: reshape / permute + cast
    tokens_fwd      hip                             vs  aten: cat + add
    tokens_bwd      hip                             vs  aten: the autograd of cat + add
                                                        (slice copy + two batch sums)
    ln_bwd_dsum     layernorm_bwd(dsum=...)         vs  layernorm_bwd, then an ATen add

All candidates run in ONE process on the same buffers, alternated ``--reps`` times (at least
four); a timed loop is ``--iters`` calls between two device events after ``--warmup`` untimed
calls, and the shader clock is sampled meanwhile (mipipe/obs/clocks.py).  Per candidate: the µs
per call of every alternation, the median, the bytes the operation has to move (every element it
touches read once and written once) and the TB/s that gives.  The working sets (77–155 MB) fit the
256 MB memory-side cache, so back-to-back calls read partly from it: an upper bound for a training
step, as for ``tools/mix_bench.py``.

Usage: python tools/vit_bench.py [--reps 4] [--iters 20] [--out profiles/vit_kernels.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

VERSUS = {"patchify/hip": "patchify/aten", "tokens_fwd/hip": "tokens_fwd/aten",
          "tokens_bwd/hip": "tokens_bwd/aten", "ln_bwd_dsum/hip": "ln_bwd_dsum/ln_bwd+aten_add"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", default="256,3,224,224")
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--reps", type=int, default=4, help="alternated repetitions (>= 4)")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed loop")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls per candidate")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    a.reps = max(a.reps, 4)

    import torch
    from mipipe.obs.clocks import ClockSampler
    from mipipe.ops import kernels as K
    from mipipe.ops._native import load_error, native_available

    if not torch.cuda.is_available():
        print("vit_bench: no GPU (a timing taken on the CPU says nothing)", file=sys.stderr)
        return 2
    if not native_available():
        print(f"vit_bench: mipipe._C is not built: {load_error()!r}", file=sys.stderr)
        return 2

    B, C, H, W = (int(v) for v in a.shape.split(","))
    P, D = a.patch, a.hidden
    N = (H // P) * (W // P)
    S = N + 1
    bf = torch.bfloat16
    torch.manual_seed(0)
    x = torch.randn(B, C, H, W, device="cuda")
    e = torch.randn(B * N, D, device="cuda").to(bf)
    cls = torch.randn(D, device="cuda")
    pos = torch.randn(S * D, device="cuda")
    dh = torch.randn(B * S, D, device="cuda").to(bf)
    dsum = torch.randn(B * S, D, device="cuda").to(bf)
    gamma = torch.rand(D, device="cuda") + 0.5
    beta = torch.randn(D, device="cuda")
    _, mean, rstd, _ = K.layernorm_fwd(dh, gamma, beta, 1e-6)
    dpos, dcls = torch.zeros(S * D, device="cuda"), torch.zeros(D, device="cuda")
    gacc, bacc = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")

    def aten_patchify():
        return x.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5) \
            .reshape(B * N, C * P * P).to(bf)

    def aten_tokens_fwd():
        c = cls.to(bf).view(1, 1, D).expand(B, 1, D)
        return (torch.cat([c, e.view(B, N, D)], 1).float() + pos.view(1, S, D)).to(bf)

    def aten_tokens_bwd():
        g = dh.view(B, S, D)
        de = g[:, 1:].contiguous()
        dp = g.sum(0, dtype=torch.float32)
        dpos.add_(dp.view(-1))
        dcls.add_(dp[0])
        return de

    def ln_then_add():
        dx = K.layernorm_bwd(dh, dh, mean, rstd, gamma, (gacc, bacc))[0]
        return dx.add_(dsum)

    act = B * S * D * 2  # one bf16 pass over the token stream
    cands = {
        "patchify/hip": (lambda: K.patchify(x, P, bf), x.numel() * 4 + x.numel() * 2),
        "patchify/aten": (aten_patchify, x.numel() * 4 + x.numel() * 2),
        "tokens_fwd/hip": (lambda: K.tokens_assemble_fwd(e, cls, pos), e.numel() * 2 + act),
        "tokens_fwd/aten": (aten_tokens_fwd, e.numel() * 2 + act),
        "tokens_bwd/hip": (lambda: K.tokens_assemble_bwd(dh, B, dpos, dcls), act + e.numel() * 2),
        "tokens_bwd/aten": (aten_tokens_bwd, act + e.numel() * 2),
        # dy, x and dsum read, dx written
        "ln_bwd_dsum/hip": (lambda: K.layernorm_bwd(dh, dh, mean, rstd, gamma, (gacc, bacc),
                                                    dsum=dsum), 4 * act),
        "ln_bwd_dsum/ln_bwd+aten_add": (ln_then_add, 4 * act),
        "ln_bwd/plain": (lambda: K.layernorm_bwd(dh, dh, mean, rstd, gamma, (gacc, bacc)),
                         3 * act),
    }
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    for fn, _ in cands.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in cands}
    with ClockSampler(0) as cs:
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
    for k, (_, by) in cands.items():
        med = statistics.median(us[k])
        rec = {"candidate": k, "us_per_call": round(med, 2),
               "us_all": [round(v, 2) for v in us[k]], "bytes_min": by,
               "TB_per_s": round(by / med / 1e6, 3)}
        if k in VERSUS:
            ref = us[VERSUS[k]]
            rec["vs"] = VERSUS[k]
            rec["speedup"] = round(statistics.median(ref) / med, 3)
            rec["faster_in_every_alternation"] = all(h < r for h, r in zip(us[k], ref))
        emit(rec)
    emit({"image": [B, C, H, W], "patch": P, "tokens": [B * S, D], "gpu_clocks": cs.summary(),
          "reps": a.reps, "iters": a.iters})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
