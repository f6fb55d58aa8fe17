"""LARS / LAMB kernels (csrc/kernels/optim.hip) on the MI355X vs the per-tensor float64 reference,
clipping, the device-side LR schedule, determinism and hipGraph replay.
Run on an MI355X:  python -m pytest tests -m gpu
"""
import copy

import pytest
import torch

from mipipe.ops._native import native, native_available
from mipipe.optim import LAMB, LARS, LRSchedule

import large_batch_common as C
from large_batch_common import rel_err

pytestmark = pytest.mark.gpu

# test_sgd_and_adamw's bounds.  Four steps need no looser ones: the fp32 _ref against the fp64
# _ref on these inputs (CPU, 4 steps) is at most 1.2e-7 on p, 6.2e-7 on LARS's m, 1.2e-7 on
# LAMB's m / v and 1.3e-7 on the gradient norm — four times that is still below each bound.
TOL_P = {"lars": 1e-6, "lamb": 1e-5}
TOL_M = {"lars": 1e-6, "lamb": 1e-5}
TOL_R = 1e-5  # trust ratios and the global norm

HPS = {"lars": C.lars_hp(), "lars_clip": C.lars_hp(max_norm=0.5, grad_scale=0.5),
       "lamb": C.lamb_hp(), "lamb_clip": C.lamb_hp(max_norm=1.0)}
GRADS = C.make_grads(4, scale=30.0)
_REF = {}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native_available(), "mipipe._C must be built for GPU tests (no silent fallback)"
    yield


def ref_for(name, steps):
    """The float64 per-tensor reference of HPS[name], computed once per (case, steps)."""
    if (name, steps) not in _REF:
        _REF[(name, steps)] = C.run_ref(C.make_params(), GRADS[:steps], HPS[name])
    return _REF[(name, steps)]


def check_against_ref(name, steps):
    hp, ref = HPS[name], ref_for(name, steps)
    got, opt = C.run_opt(C.make_params("cuda"), GRADS[:steps], hp)
    kind = hp["kind"]
    errs = dict(p=rel_err(got["p"], ref["p"]), m=rel_err(got["m"], ref["m"]),
                v=rel_err(got["v"], ref["v"]) if kind == "lamb" else 0.0)
    print(name, steps, errs)
    assert errs["p"] < TOL_P[kind] and errs["m"] < TOL_M[kind] and errs["v"] < TOL_M[kind], errs
    for k in range(steps):
        r, rr = got["ratios"][k], ref["ratios"][k]
        assert rel_err(r, rr) < TOL_R
        assert ((r - rr).abs() <= TOL_R * rr.abs()).all()  # each ratio, not only the largest
        if got["norms"][k] is not None:
            assert abs(got["norms"][k] - ref["norms"][k]) < TOL_R * ref["norms"][k]
    assert (got["norms"][0] is None) == (name == "lamb")  # LAMB takes no norm without clipping
    r = got["ratios"][0]
    one_d = [i for i, s in enumerate(C.shapes()) if len(s) == 1]
    assert r[C.I_ZERO_W] == 1.0 and all(r[i] == 1.0 for i in one_d) and r[C.I_BIG] != 1.0
    sp = opt.space
    assert torch.equal(sp.shadow, sp.flat.to(torch.bfloat16))
    assert opt.sync_step() == steps
    return opt


@pytest.mark.parametrize("name", list(HPS))
def test_native_one_step_matches_fp64_ref(name):
    check_against_ref(name, 1)


@pytest.mark.parametrize("name", list(HPS))
def test_native_four_steps_match_fp64_ref_and_padding_stays_zero(name):
    opt = check_against_ref(name, 4)
    pad = C.padding_mask(opt.space).cuda()
    assert int(pad.sum()) == 2 * 48 + 27 + 28 + 63  # two reserved pad rows, three alignment tails
    for buf in [opt.space.flat, opt.space.shadow] + list(opt._flat.values()):
        assert not buf[pad].any()
    assert all(n in opt._flat for n in (["momentum_buffer"] if name.startswith("lars")
                                        else ["exp_avg", "exp_avg_sq"]))


@pytest.mark.parametrize("kind", ["lars", "lamb"])
@pytest.mark.parametrize("max_norm,clips", [(50.0, True), (1000.0, False)])
def test_grad_norm_matches_clip_grad_norm(kind, max_norm, clips):
    hp = (C.lars_hp if kind == "lars" else C.lamb_hp)(max_norm=max_norm)
    gs64 = [torch.nn.Parameter(torch.zeros_like(g, dtype=torch.float64)) for g in GRADS[0]]
    for q, g in zip(gs64, GRADS[0]):
        q.grad = g.double().clone()
    total = float(torch.nn.utils.clip_grad_norm_(gs64, max_norm))
    assert (total > max_norm) == clips
    got, opt = C.run_opt(C.make_params("cuda"), GRADS[:1], hp)
    assert abs(float(opt.last_grad_norm()) - total) < TOL_R * total
    # the clipped gradients are what the update used
    ref = C.run_ref(C.make_params(), GRADS[:1], hp)
    assert rel_err(got["p"], ref["p"]) < TOL_P[kind]
    assert rel_err(got["m"], ref["m"]) < TOL_M[kind]
    clip = float(opt._scal[1])
    assert (clip < 1.0) == clips and abs(clip - min(1.0, max_norm / (total + 1e-6))) < 1e-6


def test_lars_without_ratio_is_the_sgd_kernel():
    params = C.make_params("cuda")
    opt = LARS(params, 0.1, momentum=0.9, weight_decay=1e-4, trust_coefficient=None,
               exclude_1d=False)
    p2 = opt.space.flat.clone()
    m2 = torch.zeros_like(p2)
    sh2 = torch.empty_like(opt.space.shadow)
    for k in range(3):
        C.set_grads(opt, params, GRADS[k])
        native().sgd_step(p2, opt.space.flat_grad, m2, sh2, 0.1, 0.9, 0.0, 1e-4, False, k == 0, 1.0)
        opt.step()
        assert opt.last_grad_norm() is None  # two launches: no norm pass
    assert rel_err(opt.space.flat, p2) < 1e-6
    assert rel_err(opt._flat["momentum_buffer"], m2) < 1e-6
    assert torch.equal(opt.last_trust_ratios(), torch.ones(C.NSEG, device="cuda"))
    assert float(opt.last_lr()) == pytest.approx(0.1, rel=1e-7)


@pytest.mark.parametrize("kind", ["constant", "linear", "poly", "cosine"])
def test_device_lr_follows_the_schedule(kind):
    base, end, W, T = 0.3, 0.02, 3, 9
    sched = LRSchedule(kind, base, W, T, end)
    params = C.make_params("cuda")
    opt = LARS(params, sched, max_grad_norm=1.0) if kind in ("constant", "poly") \
        else LAMB(params, sched)
    C.set_grads(opt, params, GRADS[0])
    dev = []
    for k in range(T + 3):
        opt.step()
        dev.append(opt.last_lr().clone())
    dev = torch.stack(dev).cpu().double()
    want = torch.tensor([sched.lr_at(k) for k in range(T + 3)], dtype=torch.float64)
    print(kind, (dev - want).abs().max().item())
    assert ((dev - want).abs() <= 1e-6 * base).all(), (dev, want)
    assert opt.sync_step() == T + 3 and opt.current_lr() == sched.lr_at(T + 3)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", ["lars_clip", "lamb_clip"])
def test_two_runs_are_bit_identical(name, det):
    from mipipe.ops.determinism import deterministic
    with deterministic(det):
        a, oa = C.run_opt(C.make_params("cuda"), GRADS[:3], HPS[name])
        b, ob = C.run_opt(C.make_params("cuda"), GRADS[:3], HPS[name])
    for key in ("p", "m", "v"):
        assert torch.equal(a[key], b[key]), key
    assert all(torch.equal(x, y) for x, y in zip(a["ratios"], b["ratios"]))
    assert a["norms"] == b["norms"]
    assert torch.equal(oa.space.shadow, ob.space.shadow)


def _graph_vs_eager(models, opts, step_fn, batch, steps=5):
    from mipipe.train.graph import GraphedStep, graph_safe
    ok, why = graph_safe(models[1], opts[1])
    assert ok, why
    eager_lr = []
    for _ in range(steps):
        step_fn(models[0], opts[0])(*batch)
        eager_lr.append(float(opts[0].last_lr()))
    gs = GraphedStep(step_fn(models[1], opts[1]), batch, warmup=1, inputs=[batch])
    replay_lr = [float(opts[1].last_lr())]
    for _ in range(steps - 1):
        gs.replay(0)
        replay_lr.append(float(opts[1].last_lr()))
    torch.cuda.synchronize()
    assert opts[0].sync_step() == steps and opts[1].sync_step() == steps
    assert replay_lr == eager_lr and len(set(replay_lr[1:])) > 1, (replay_lr, eager_lr)
    sched = opts[1].schedule
    assert replay_lr == pytest.approx([sched.lr_at(k) for k in range(steps)], rel=1e-5)
    for (n, p), (_, q) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(p, q), n
    assert torch.equal(opts[0].last_trust_ratios(), opts[1].last_trust_ratios())
    assert torch.isfinite(opts[1].space.flat).all()


def test_graphed_resnet18_lars_step_equals_eager():
    from mipipe.models import create_model
    from mipipe.ops.determinism import deterministic
    from mipipe.ops.functional import cross_entropy
    with deterministic(True):
        torch.manual_seed(0)
        a = create_model("resnet18", num_classes=10).cuda()
        models = [a, copy.deepcopy(a)]
        opts = [LARS(m.parameters(), LRSchedule("poly", 0.5, 2, 6), momentum=0.9,
                     weight_decay=1e-4, trust_coefficient=0.02) for m in models]
        x = torch.randn(8, 3, 32, 32, device="cuda")
        y = torch.randint(0, 10, (8,), device="cuda")

        def step_fn(m, o):
            def step(xx, yy):
                o.zero_grad()
                loss = cross_entropy(m(xx), yy)
                loss.backward()
                o.step()
                return loss
            return step

        _graph_vs_eager(models, opts, step_fn, (x, y))
    r = opts[1].last_trust_ratios()
    assert (r != 1.0).any() and (r == 1.0).any()  # conv / fc adapted, BN and biases not


def test_graphed_bert_tiny_lamb_clip_step_equals_eager():
    from mipipe.models import create_model
    from mipipe.ops.determinism import deterministic
    with deterministic(True):
        torch.manual_seed(0)
        a = create_model("bert_tiny").cuda()
        models = [a, copy.deepcopy(a)]
        opts = [LAMB(m.parameters(), LRSchedule("linear", 2e-3, 2, 8), max_grad_norm=1.0)
                for m in models]
        B, S, P, V = 2, 128, 20, a.config.vocab_size
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        ids = torch.randint(0, V, (B, S), device="cuda", generator=g)
        am = torch.ones(B, S, device="cuda", dtype=torch.int64)
        pos = torch.stack([torch.randperm(S, device="cuda", generator=g)[:P] for _ in range(B)])
        labels = torch.randint(0, V, (B, P), device="cuda", generator=g)

        def step_fn(m, o):
            def step(i, msk, ps, lb):
                o.zero_grad()
                loss = m(i, msk, masked_positions=ps, labels=lb)
                loss.backward()
                o.step()
                return loss
            return step

        _graph_vs_eager(models, opts, step_fn, (ids, am, pos, labels))
    assert float(opts[1].last_grad_norm()) > 0
