"""bench.py's driver contract on the CPU: `python bench.py --gpus N` spawns its own N ranks
(task.py:117-124's one-process-per-GPU), every rank checks the process-group size, rank 0
prints exactly one JSON line with n_gpus = N.  gloo stands in for RCCL here."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
CPU_ARGS = ["--device", "cpu", "--model", "mnist_cnn", "--res", "28", "--classes", "10",
            "--batch", "8", "--steps", "2", "--warmup", "1"]


def _env(**kw):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e["OMP_NUM_THREADS"] = "1"  # single-threaded CPU kernels: run-to-run identical sums
    e.update(kw)
    return e


def _json_lines(out: str):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("n", [1, 2])
def test_bench_self_spawn_gloo(n):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n)] + CPU_ARGS, env=_env(),
                       capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout  # only rank 0 prints to stdout
    j = lines[0]
    assert j["n_gpus"] == n and j["config"]["parallelism"] == f"dp{n}"
    assert j["config"]["global_batch"] == 8 * n
    assert j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0
    if n > 1:
        from mipipe.ops._native import native_available
        assert j["config"]["native_reducer"] == native_available()
        assert j["config"]["rccl"]["TORCH_NCCL_HIGH_PRIORITY"] == "1"


def test_bench_force_reduce_world1_gloo():
    """--force-reduce wraps in DDP and issues the collectives at world size 1."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--force-reduce"] + CPU_ARGS,
                       env=_env(MASTER_ADDR="127.0.0.1", MASTER_PORT="0", WORLD_SIZE="1",
                                RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    j = _json_lines(r.stdout)[0]
    assert j["config"]["force_reduce"] is True and j["n_gpus"] == 1


def test_bench_rejects_world_mismatch():
    """A launcher that started fewer ranks than --gpus must not yield a silent 1-rank number."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4"] + CPU_ARGS,
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120, cwd="/tmp")
    assert r.returncode != 0
    assert _json_lines(r.stdout) == []


def test_spawn_local_ranks_fail_fast(tmp_path):
    from mipipe.launch.local import spawn_local_ranks
    script = tmp_path / "s.py"
    script.write_text(
        "import os, sys, time\n"
        "r = int(os.environ['RANK'])\n"
        "assert os.environ['WORLD_SIZE'] == '3' and os.environ['LOCAL_RANK'] == str(r)\n"
        "if r == 1: sys.exit(7)\n"
        "time.sleep(60)\n")
    import time
    t0 = time.time()
    rc = spawn_local_ranks([sys.executable, str(script)], 3, grace=2.0)
    assert rc == 7
    assert time.time() - t0 < 30  # the sleeping ranks were terminated


def test_spawn_local_ranks_env_contract():
    from mipipe.launch.local import rank_envs
    envs = rank_envs(4, port=12345)
    assert [e["RANK"] for e in envs] == ["0", "1", "2", "3"]
    assert all(e["WORLD_SIZE"] == "4" and e["MASTER_ADDR"] == "127.0.0.1"
               and e["MASTER_PORT"] == "12345" and e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
               for e in envs)


@pytest.mark.parametrize("comm", ["fp32", "bf16"])
def test_bench_world4_gloo_matches_global_batch(tmp_path, comm):
    """`bench.py --gpus 4` (4 gloo ranks, mipipe DDP) ends with bit-identical parameters on
    every rank, equal (to fp32 reduction-order noise) to ONE process that runs the same four
    per-rank batches and averages their gradients (--emulate-ranks 4): the DDP contract of the
    reference's task.py:189 (average of per-rank gradients, rank 0's BN buffers broadcast before
    every forward), rehearsed at world 4 before any 8-GPU run."""
    import torch
    args = ["--device", "cpu", "--model", "mnist_cnn", "--res", "28", "--classes", "10",
            "--batch", "8", "--steps", "3", "--warmup", "1"]
    d4, d1 = tmp_path / "w4", tmp_path / "w1"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dump-params", str(d4),
                        "--comm-dtype", comm] + args,
                       env=_env(), capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--emulate-ranks", "4",
                        "--dump-params", str(d1)] + args,
                       env=_env(), capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    ranks = [torch.load(d4 / f"rank{i}.pt", weights_only=True) for i in range(4)]
    ref = torch.load(d1 / "rank0.pt", weights_only=True)
    for rk in ranks[1:]:
        for a, b in zip(ranks[0]["params"], rk["params"]):
            assert torch.equal(a, b)
    moved = 0.0
    # fp32 wire: reduction-order noise only (~3e-8): a race between the per-forward buffer
    # broadcast and the BN statistics shift showed up here as 1e-5..2e-4 run-to-run noise.
    # bf16 wire: gradients rounded to 8 bits before the sum; 4 SGD steps at lr 0.1 move a
    # parameter by <= ~1e-3 relative of its update.
    tol = dict(rtol=1e-5, atol=1e-6) if comm == "fp32" else dict(rtol=1e-3, atol=2e-4)
    for a, b in zip(ranks[0]["params"], ref["params"]):
        assert torch.allclose(a, b, **tol), (a - b).abs().max()
        moved += float((a - b).abs().max())
    for a, b in zip(ranks[0]["buffers"], ref["buffers"]):
        btol = dict(rtol=1e-4, atol=1e-5) if comm == "fp32" else dict(rtol=1e-2, atol=1e-3)
        assert torch.allclose(a.float(), b.float(), **btol)


def test_rccl_profiles_env():
    """MIPIPE_RCCL_PROFILE channel profiles: applied as defaults (the environment wins), the
    high-priority comm stream always, unknown names rejected; the settings report lists them."""
    from mipipe.parallel.dist_utils import configure_rccl_env, rccl_settings
    e = configure_rccl_env({})
    assert e["TORCH_NCCL_HIGH_PRIORITY"] == "1" and "NCCL_MAX_NCHANNELS" not in e
    e = configure_rccl_env({"MIPIPE_RCCL_PROFILE": "overlap"})
    assert e["NCCL_MAX_NCHANNELS"] == "8"
    e = configure_rccl_env({"NCCL_MIN_NCHANNELS": "4"}, profile="bandwidth")
    assert e["NCCL_MIN_NCHANNELS"] == "4"  # explicit setting kept
    with pytest.raises(ValueError):
        configure_rccl_env({}, profile="fastest")
    rep = rccl_settings({"NCCL_MIN_NCHANNELS": "32", "PATH": "/bin", "TORCH_NCCL_HIGH_PRIORITY": "1"})
    assert rep == {"NCCL_MIN_NCHANNELS": "32", "TORCH_NCCL_HIGH_PRIORITY": "1"}


def test_bench_world4_gloo_bert_matches_emulated_ranks(tmp_path):
    """`bench.py --gpus 4 --model bert_tiny` (4 gloo ranks, mipipe DDP with the tied word
    embedding's lookup gradient exchanged as sparse (id, row) pairs) ends with bit-identical
    parameters on every rank, equal to one process that runs the four per-rank batches and
    averages their gradients (--emulate-ranks 4)."""
    import torch
    args = ["--device", "cpu", "--model", "bert_tiny", "--batch", "2", "--seq", "32",
            "--steps", "2", "--warmup", "1", "--bert-dropout", "0"]
    d4, d1 = tmp_path / "w4", tmp_path / "w1"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dump-params", str(d4)] + args,
                       env=_env(), capture_output=True, text=True, timeout=900, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--emulate-ranks", "4",
                        "--dump-params", str(d1)] + args,
                       env=_env(), capture_output=True, text=True, timeout=900, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    ranks = [torch.load(d4 / f"rank{i}.pt", weights_only=True) for i in range(4)]
    ref = torch.load(d1 / "rank0.pt", weights_only=True)
    for rk in ranks[1:]:
        for a, b in zip(ranks[0]["params"], rk["params"]):
            assert torch.equal(a, b)
    for a, b in zip(ranks[0]["params"], ref["params"]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max()


def _dump(d):
    import numpy as np
    assert sorted(os.listdir(d)) == ["buffers.npy", "loss.npy"]
    out = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    for v in out.values():
        assert v.dtype == np.float32 and v.ndim == 1 and v.size > 0 and np.isfinite(v).all()
    return out


def test_bench_dump_outputs_is_first_step_and_plain_run_is_lean(tmp_path):
    """`--dump-outputs DIR`: after the timed steps the run is put back into its initial state and
    the timed step is called once more on batch 0; the loss it returns and the buffers it leaves
    are written as float32 .npy files.  Checked against an independent value: a run of ONE timed
    step without warm-up reports that very step as final_loss and (--dump-params) leaves its
    buffers, and the single-threaded CPU kernels are exact, so the dump must equal both; a run
    with other --steps / --warmup writes the same dump, and its own final_loss is untouched by
    the extra call.  A plain run (no `--full`) times the headline only, and asking for an extra
    timed run without `--full` is an error, not a silent no-op."""
    import numpy as np
    import torch
    outs, lines = [], []
    for d, steps, warm in ((tmp_path / "a", 1, 0), (tmp_path / "b", 3, 1)):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dump-outputs", str(d),
                            "--dump-params", str(tmp_path / f"p{steps}")] + CPU_ARGS
                           + ["--steps", str(steps), "--warmup", str(warm)], env=_env(),
                           capture_output=True, text=True, timeout=300, cwd="/tmp")
        assert r.returncode == 0, r.stderr[-3000:]
        j = _json_lines(r.stdout)[0]
        assert j["steps"] == steps and j["ms_per_step"] > 0
        assert "reference_config" not in j and "deterministic_variant" not in j
        outs.append(_dump(d))
        lines.append(j)
    first = torch.load(tmp_path / "p1" / "rank0.pt", weights_only=True)
    assert float(outs[0]["loss"][0]) == np.float32(lines[0]["final_loss"])
    assert np.array_equal(outs[0]["buffers"],
                          torch.cat([b.float().reshape(-1) for b in first["buffers"]]).numpy())
    for f, v in outs[0].items():
        assert np.array_equal(v, outs[1][f]), f
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + CPU_ARGS
                       + ["--steps", "3", "--warmup", "1"], env=_env(),
                       capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    assert _json_lines(r.stdout)[0]["final_loss"] == lines[1]["final_loss"] != lines[0]["final_loss"]
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--reference-config", "on"]
                       + CPU_ARGS, env=_env(), capture_output=True, text=True, timeout=120,
                       cwd="/tmp")
    assert r.returncode == 2 and "--full" in r.stderr and _json_lines(r.stdout) == []


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_timed_step_gpu(tmp_path):
    """On the GPU the dump comes from the timed callable itself: the hipGraph replay with the
    run's float-atomic kernels and tuned plans, after the reset to the initial state.  The
    independent value is a second process that runs ONE eager step (--graph off, heuristic
    plans, no warm-up) from the same seed: its final_loss is that first step's loss and its dump
    repeats it.  Neither is bit-reproducible (atomics), so they are compared to one bf16 ulp
    (2^-8 relative): the loss is a mean over 64 samples of values computed through bf16
    activations whose roundings (2^-9 each) are independent, and the BatchNorm statistics are
    fp32 means of such activations, compared in relative L2 norm."""
    import numpy as np
    R18 = ["--model", "resnet18", "--res", "32", "--batch", "64", "--gpus", "1"]
    outs, lines = [], []
    for d, extra in ((tmp_path / "g", ["--steps", "2", "--warmup", "1"]),
                     (tmp_path / "e", ["--steps", "1", "--warmup", "0", "--graph", "off",
                                       "--tune", "0"])):
        r = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(d)] + R18 + extra,
                           env=_env(), capture_output=True, text=True, timeout=240, cwd="/tmp")
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(_json_lines(r.stdout)[0])
        outs.append(_dump(d))
    assert lines[0]["config"]["hip_graph"] is True and lines[0]["config"]["deterministic"] is False
    assert lines[1]["config"]["hip_graph"] is False
    ulp = 2.0 ** -8
    first = lines[1]["final_loss"]
    print("first eager step", first, "dumped: graph", outs[0]["loss"], "eager", outs[1]["loss"])
    assert abs(float(outs[0]["loss"][0]) - first) <= ulp * first
    assert abs(float(outs[1]["loss"][0]) - first) <= ulp * first
    g, e = outs[0]["buffers"].astype(np.float64), outs[1]["buffers"].astype(np.float64)
    rel = np.linalg.norm(g - e) / np.linalg.norm(e)
    print("buffers relative L2 distance", rel)
    assert g.shape == e.shape and rel <= ulp
    # the step really ran: BatchNorm running means left 0, running variances left 1
    assert np.count_nonzero((g != 0) & (g != 1)) > g.size // 2


def test_bench_reference_config_block_gloo():
    """`--full --reference-config on` times the reference's config of record (ResNet-18 32x32,
    1000 classes, fp32, deterministic) after the headline in the same process (and, here, under
    a 2-rank gloo DDP), and reports it inside the ONE JSON line."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--full", "--reference-config", "on",
                        "--time-deterministic", "on", "--ref-batch", "4"] + CPU_ARGS, env=_env(),
                       capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    j = lines[0]
    assert j["config"]["model"] == "mnist_cnn" and j["n_gpus"] == 2
    ref = j["reference_config"]
    assert ref["model"] == "resnet18" and ref["classes"] == 1000 and ref["image_size"] == 32
    assert ref["dtype"] == "fp32" and ref["deterministic"] is True
    assert ref["batch_per_gpu"] == 4 and ref["global_batch"] == 8
    assert ref["value"] > 0 and ref["ms_per_step"] > 0 and ref["steps"] == 2
    det = j["deterministic_variant"]
    assert det["deterministic"] is True and det["value"] > 0 and det["steps"] == 2
    assert j["config"]["deterministic"] is False
