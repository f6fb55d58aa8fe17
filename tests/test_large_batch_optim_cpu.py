"""LARS / LAMB / LRSchedule on the CPU path: chunk tables, the optimizers vs the per-tensor float64
reference, edge cases, the schedule, checkpoints, task.py flags and a 2-rank gloo DDP run."""
import copy
import json
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from mipipe.optim import LAMB, LARS, SGD, LRSchedule
from mipipe.optim.large_batch import CHUNK, build_tables

import large_batch_common as C
from large_batch_common import rel_err

# fp32 per-tensor rules against the same rules in float64, 4 steps: fp32 rounding (6e-8) through
# a few hundred thousand-element sums and four updates stays two orders below this
TOL = 1e-5


def test_chunk_table_tiles_every_segment():
    params = C.make_params()
    opt = LARS(params, 0.1)
    ranges = opt.space.ranges()
    assert len(ranges) == C.NSEG
    sizes = sorted(b - a for a, b, _ in ranges)
    assert sizes[0] == 64 and CHUNK + 64 in sizes and 65 * CHUNK in sizes
    assert CHUNK == C.CH
    wd = [0.1 * i for i in range(len(ranges))]
    chunks, segs = build_tables([(a, b) for a, b, _ in ranges], wd, [i % 2 for i in range(len(wd))])
    assert chunks.dtype == torch.int32 and segs.dtype == torch.int32
    assert torch.equal(segs[:, 0].contiguous().view(torch.float32), torch.tensor(wd))
    assert segs[:, 1].tolist() == [i % 2 for i in range(len(wd))]
    nxt = 0
    for s, (a, b, p) in enumerate(ranges):
        first, cnt = int(segs[s, 2]), int(segs[s, 3])
        assert first == nxt and cnt == -(-(b - a) // CHUNK)
        pos = a
        for seg, off64, ln, _ in chunks[first:first + cnt].tolist():
            assert seg == s and off64 * 64 == pos  # in order, no gap, no overlap
            assert ln % 64 == 0 and 0 < ln <= CHUNK
            pos += ln
        assert pos == b  # the whole reserved range, padding and pad rows included, never beyond
        nxt = first + cnt
    assert nxt == chunks.shape[0]
    padded = [(a, b, p) for a, b, p in ranges if getattr(p, "_mipipe_pad_rows", None)]
    assert len(padded) == 1 and padded[0][1] - padded[0][0] == C.PAD_ROWS * 48
    # the optimizer's own tables are these, with its weight decay / adapt columns
    assert torch.equal(opt._chunks.cpu(), chunks)
    with pytest.raises(ValueError):
        build_tables([(0, 100)], [0.0], [True])


@pytest.mark.parametrize("hp", [C.lars_hp(), C.lars_hp(max_norm=0.5, grad_scale=0.5),
                                C.lars_hp(exclude_1d=False), C.lamb_hp(),
                                C.lamb_hp(max_norm=1.0), C.lamb_hp(exclude_1d=False)],
                         ids=["lars", "lars_clip", "lars_all", "lamb", "lamb_clip", "lamb_all"])
def test_optimizer_matches_per_tensor_ref(hp):
    params = C.make_params()
    grads = C.make_grads(4, scale=30.0)
    ref = C.run_ref(params, grads, hp)
    got, opt = C.run_opt(params, grads, hp)
    assert rel_err(got["p"], ref["p"]) < TOL
    assert rel_err(got["m"], ref["m"]) < TOL
    if hp["kind"] == "lamb":
        assert rel_err(got["v"], ref["v"]) < TOL
    for k in range(4):
        assert torch.isfinite(got["ratios"][k]).all()
        assert rel_err(got["ratios"][k], ref["ratios"][k]) < TOL
        if got["norms"][k] is not None:
            assert abs(got["norms"][k] - ref["norms"][k]) < TOL * ref["norms"][k]
    if hp["max_norm"] is not None:
        assert all(n is not None for n in got["norms"])
        assert ref["norms"][0] * hp["grad_scale"] > hp["max_norm"] or hp["kind"] == "lamb"
    # edge cases: zero gradient / zero weight -> ratio 1 and no NaN; 1-D -> ratio 1, no decay
    r = got["ratios"][0]
    assert r[C.I_ZERO_W] == 1.0
    if hp["kind"] == "lars":
        assert r[C.I_ZERO_G] == 1.0
    one_d = [i for i, s in enumerate(C.shapes()) if len(s) == 1]
    if hp["exclude_1d"]:
        assert all(r[i] == 1.0 for i in one_d)
    else:
        assert any(r[i] != 1.0 for i in one_d)
    assert r[C.I_BIG] != 1.0 and torch.isfinite(got["p"]).all()
    assert opt.sync_step() == 4 and opt.param_groups[0]["step"] == 4
    # padding (alignment tails, pad rows) is still exactly zero everywhere
    pad = C.padding_mask(opt.space)
    assert pad.sum() > 0
    for buf in [opt.space.flat] + list(opt._flat.values()):
        assert not buf[pad].any()


def test_excluded_1d_takes_no_decay():
    """A 1-D tensor with zero gradient does not move under exclude_1d (no decay), and does
    without it."""
    for excl in (True, False):
        params = C.make_params()
        before = params[5].detach().clone()
        grads = C.make_grads(1)
        grads[0][5].zero_()
        C.run_opt(params, grads, C.lars_hp(exclude_1d=excl, weight_decay=0.1))
        assert torch.equal(params[5].detach(), before) == excl


@pytest.mark.parametrize("kind", ["constant", "linear", "poly", "cosine"])
def test_schedule_formula(kind):
    base, end, W, T = 0.8, 0.05, 4, 20
    s = LRSchedule(kind, base, W, T, end)
    lrs = [s.lr_at(k) for k in range(T + 3)]
    assert all(math.isfinite(v) for v in lrs)
    for k in range(W):
        assert lrs[k] == pytest.approx(base * (k + 1) / W, rel=1e-14)
    assert lrs[W - 1] == pytest.approx(base, rel=1e-14)  # warm-up ends at the base rate
    assert lrs[W] == pytest.approx(base, rel=1e-14)      # x = 0
    mid = W + (T - W) // 2                               # x = 1/2
    want_mid = {"constant": base, "linear": end + (base - end) * 0.5,
                "poly": end + (base - end) * 0.25, "cosine": end + (base - end) * 0.5}[kind]
    assert lrs[mid] == pytest.approx(want_mid, rel=1e-12)
    want_end = base if kind == "constant" else end
    for k in (T, T + 1, T + 2):                          # x clamped to 1
        assert lrs[k] == pytest.approx(want_end, rel=1e-12, abs=1e-15)
    if kind != "constant":
        assert all(a > b for a, b in zip(lrs[W:T], lrs[W + 1:T + 1]))  # strictly decaying
    with pytest.raises(ValueError):
        LRSchedule("step", 0.1)


@pytest.mark.parametrize("hp", [C.lars_hp(max_norm=0.5), C.lamb_hp(max_norm=1.0)],
                         ids=["lars", "lamb"])
def test_checkpoint_resume_is_bit_identical(hp):
    grads = C.make_grads(5, scale=30.0)
    straight, o_s = C.run_opt(C.make_params(), grads, hp)
    params = C.make_params()
    _, o1 = C.run_opt(params, grads[:3], hp)
    sd = copy.deepcopy(o1.state_dict())
    assert sd["param_groups"][0]["step"] == 3 and sd["param_groups"][0]["lr_schedule"] == hp["sched"][0]
    name = "momentum_buffer" if hp["kind"] == "lars" else "exp_avg_sq"
    assert name in sd["state"][0]
    params2 = [torch.nn.Parameter(p.detach().clone()) for p in params]
    params2[C.I_PAD]._mipipe_pad_rows = C.PAD_ROWS
    o2 = C.make_opt(params2, dict(hp, sched=("constant", 9.0, 0, 0, 0.0)))
    o2.load_state_dict(sd)
    assert o2.sync_step() == 3
    assert o2.current_lr() == o1.current_lr() == LRSchedule(*hp["sched"]).lr_at(3)
    resumed, _ = C.run_opt(params2, grads[3:], hp, opt=o2)
    assert torch.equal(resumed["p"], straight["p"])
    assert torch.equal(resumed["m"], straight["m"]) and torch.equal(resumed["v"], straight["v"])
    assert o2.sync_step() == 5 and o2.current_lr() == o_s.current_lr()
    o2.reset_state()
    assert o2.sync_step() == 0 and not any(t.any() for t in o2._flat.values())


def test_task_flags(tmp_path, monkeypatch):
    from mipipe.train import task as T
    monkeypatch.setenv("MIPIPE_FORCE_CPU", "1")
    monkeypatch.delenv("AIP_MODEL_DIR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mf = tmp_path / "m.json"
    args = ["--arch", "mnist_cnn", "--dataset", "mnist", "--batch_size", "32", "--train-samples",
            "96", "--test-samples", "32", "--local_training", "--model_dir", str(tmp_path / "o"),
            "--learning_rate", "0.05", "--log-every", "1", "--metrics-file", str(mf),
            "--num_epochs", "2"]
    assert T.main(args + ["--optimizer", "lars", "--lr-schedule", "poly", "--lr-warmup-steps", "2",
                          "--clip-grad-norm", "1"]) == 0
    m = json.loads(mf.read_text())
    assert m["steps"] == 6 and math.isfinite(m["loss"])
    # the last of 6 steps of poly(warm-up 2, total 2 epochs x 3 steps)
    want = LRSchedule("poly", 0.05, 2, 6).lr_at(5)
    assert m["lr"] == pytest.approx(want, rel=1e-5) and 0 < m["lr"] < 0.05
    # defaults: today's SGD, no lr in the metrics; sgd + schedule: LARS without a trust ratio
    ns = _parse(T, [])
    w = [torch.nn.Parameter(torch.randn(4, 4))]
    assert type(T._make_optimizer(ns, w, None)) is SGD
    ns2 = _parse(T, ["--lr-schedule", "cosine", "--lr-total-steps", "10"])
    o = T._make_optimizer(ns2, [torch.nn.Parameter(torch.randn(4, 4))], None)
    assert type(o) is LARS and o.param_groups[0]["trust_coefficient"] is None
    assert o.param_groups[0]["exclude_1d"] is False and o.param_groups[0]["total_steps"] == 10
    o = T._make_optimizer(_parse(T, ["--optimizer", "lamb"]),
                          [torch.nn.Parameter(torch.randn(4, 4))], None)
    assert type(o) is LAMB
    assert T.main(args[:-2] + ["--num_epochs", "1"]) == 0
    assert "lr" not in json.loads(mf.read_text())


def _parse(T, argv):
    return T.build_parser().parse_args(argv)


def _ddp_worker(rank, world, port, out):
    import torch.distributed as dist
    from mipipe import nn as mnn
    from mipipe.ops import functional as MF
    from mipipe.parallel import DistributedDataParallel
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(rank)  # different init per rank: DDP broadcasts rank 0's

    class MLP(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1 = mnn.Linear(16, 32)
            self.fc2 = mnn.Linear(32, 8)

        def forward(self, x):
            return self.fc2(self.fc1(x, act="relu"))

    m = MLP()
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.0005, first_bucket_mb=0.0001)
    opt = LAMB(ddp.parameters(), LRSchedule("linear", 0.01, 1, 3), max_grad_norm=0.5)
    g = torch.Generator().manual_seed(123)
    X = torch.randn(4 * world, 16, generator=g)
    Y = torch.randint(0, 8, (4 * world,), generator=g)
    for _ in range(3):
        opt.zero_grad()
        MF.cross_entropy(ddp(X[rank * 4:(rank + 1) * 4]), Y[rank * 4:(rank + 1) * 4]).backward()
        opt.step()
    out[rank] = (torch.cat([p.detach().reshape(-1) for p in m.parameters()]),
                 opt.last_trust_ratios().clone(), float(opt.last_grad_norm()), opt.sync_step())
    dist.destroy_process_group()


def test_ddp_gloo_lamb_ranks_bit_identical():
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_ddp_worker, args=(world, 29600 + os.getpid() % 300, out), nprocs=world, join=True)
    (f0, r0, n0, s0), (f1, r1, n1, s1) = out[0], out[1]
    assert torch.equal(f0, f1), "replicas diverged"
    assert torch.equal(r0, r1) and n0 == n1 and n0 > 0 and s0 == s1 == 3
    assert (r0 != 1.0).any() and torch.isfinite(f0).all()
