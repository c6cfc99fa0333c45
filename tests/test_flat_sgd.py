"""Flat SGD on CPU: the reference ops (sgd_step_, sgd_step_sparse_) against
each other and against torch.optim.SGD, and FlatSGD with the sparse
hand-over on vs off (OKTOPK_SPARSE_STEP) — parameters and momentum must not
change by a bit, on buckets that take the hand-over and on buckets that fall
back alike — plus its optimizer surface: param_groups, state_dict, the
fp32-only check and the Trainer / environment selection."""
import os

import pytest
import torch

from conftest import run_dist
from oktopk_amd import ops
from oktopk_amd.config import EngineConfig, OkTopkConfig
from oktopk_amd.ops import reference as ref

LR = 0.05


def _sparse_grad(n, m, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(n, generator=g)[:m].sort().values.to(torch.int32)
    val = torch.randn(m, generator=g)
    val[::11] = 0.0   # kept by tau < 0 only
    val[5::11] = -0.0
    return idx, val


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    buf = torch.randn(n, generator=g) * 0.1
    buf[::3] = -0.0   # a zero gradient must keep the sign where the formula does
    return p, buf


# -- reference ops ------------------------------------------------------------

@pytest.mark.parametrize("tau", [-1.0, 0.0, 0.9])
@pytest.mark.parametrize("gs", [None, 0.37])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_reference_sparse_step_is_densify_plus_dense_step(momentum, nesterov,
                                                          wd, gs, tau):
    total, m = 5000, 400
    idx, val = _sparse_grad(total, m, 3)
    scale = 0.5 if tau < 0 else 1.0
    gscale = None if gs is None else torch.tensor([gs])
    for base, n in [(0, total), (1234, 2000), (4000, 1000)]:
        g = ref.densify_sparse_grad(idx, val, base, n, scale, tau)
        pd, bd = _state(n, 7)
        ps, bs = _state(n, 7)
        ops.sgd_step_(pd, g, bd, LR, momentum, wd, nesterov, gscale=gscale)
        ops.sgd_step_sparse_(ps, idx, val, base, scale, tau, bs, LR, momentum,
                             wd, nesterov, gscale=gscale)
        assert torch.equal(pd.view(torch.int32), ps.view(torch.int32))
        assert torch.equal(bd.view(torch.int32), bs.view(torch.int32))
        p0, b0 = _state(n, 7)
        assert not torch.equal(pd, p0)
        if momentum == 0:  # the buffer is not touched
            assert torch.equal(bd.view(torch.int32), b0.view(torch.int32))


def test_reference_step_momentum_zero_takes_an_empty_buffer():
    p, _ = _state(100, 1)
    p0 = p.clone()
    g = torch.randn(100)
    ops.sgd_step_(p, g, torch.zeros(0), LR, 0.0, 0.0, False)
    assert torch.equal(p, p0 - g * LR)


@pytest.mark.parametrize("nesterov", [False, True])
def test_reference_step_against_torch_sgd(nesterov):
    """One step from a common state, five times, state re-synchronised after
    each comparison.  torch fuses `alpha *` into its adds, so up to six
    roundings differ between the two formulations, each relative to an
    intermediate bounded by M = (2 + mom)(|g| + wd|p|) + (1 + mom) mom |buf|:
    |dp| <= 8 * 2^-24 * (|p| + lr * M) per element."""
    n, mom, wd = 5000, 0.9, 5e-4
    gen = torch.Generator().manual_seed(13)
    p, buf = _state(n, 17)
    param = torch.nn.Parameter(p.clone())
    opt = torch.optim.SGD([param], lr=LR, momentum=mom, weight_decay=wd,
                          nesterov=nesterov, foreach=False)
    opt.state[param]["momentum_buffer"] = buf.clone()
    for _ in range(5):
        g = torch.randn(n, generator=gen)
        p0, b0 = p.clone(), buf.clone()
        param.grad = g.clone()
        opt.step()
        ops.sgd_step_(p, g, buf, LR, mom, wd, nesterov)
        big_m = (2 + mom) * (g.abs() + wd * p0.abs()) + (1 + mom) * mom * b0.abs()
        bound = 8 * 2.0 ** -24 * (p0.abs() + LR * big_m)
        err = (p.double() - param.detach().double()).abs()
        assert bool((err <= bound.double()).all()), float((err / bound).max())
        assert not torch.equal(p, p0)
        # re-synchronise on torch's state
        p.copy_(param.detach())
        buf.copy_(opt.state[param]["momentum_buffer"])


def test_clip_scale_from_sumsq_is_the_kernel_formula():
    for ss, mx in [(4.0, 1.0), (0.25, 1.0), (1e-30, 1e-3), (123.456, 0.1)]:
        acc = torch.tensor([ss], dtype=torch.float64)
        out = ops.clip_scale_from_sumsq(acc, mx)
        assert out.dtype == torch.float32 and out.shape == (1,)
        gn = ss ** 0.5
        mxf = float(torch.tensor(mx, dtype=torch.float32))
        want = torch.tensor(mxf / (gn + 1e-6) if gn > mxf else 1.0,
                            dtype=torch.float64).to(torch.float32)
        assert float(out) == float(want)


# -- engine: the per-name hand-over ------------------------------------------

def test_allreducer_records_hand_over_per_name():
    from oktopk_amd import AllReducer, Comm

    cfg = EngineConfig(compressor="oktopk", density=0.05,
                       oktopk=OkTopkConfig(dense_warmup_iters=0,
                                           global_threshold_recompute_interval=3))
    eng = AllReducer(Comm(None), cfg)
    gen = torch.Generator().manual_seed(2)
    for it in range(4):
        eng.run("a", torch.randn(2000, generator=gen), sparse_ok=True)
        sg_a = eng.sparse_result
        eng.run("b", torch.randn(900, generator=gen), sparse_ok=(it != 2))
        assert eng.sparse_results["a"] is sg_a
        assert eng.sparse_results["b"] is eng.sparse_result
        # iterations 0 and 3 are exact (dense); 2 did not ask for "b"
        assert (sg_a is not None) == (it in (1, 2))
        assert (eng.sparse_results["b"] is not None) == (it == 1)
    eng.run("a", torch.randn(2000, generator=gen), sparse_ok=True)
    assert eng.sparse_results["a"] is not None
    eng.run_many([("a", torch.randn(2000, generator=gen), None),
                  ("b", torch.randn(900, generator=gen), None)])
    assert eng.sparse_results == {"a": None, "b": None}


# -- FlatSGD, hand-over on vs off --------------------------------------------

_STEPS = 8
_GLOBAL_INTERVAL = 3


def _cfg(**kw):
    return EngineConfig.preset(
        "vgg", compressor="oktopk", density=0.01, dense_warmup_iters=0,
        local_threshold_recompute_interval=4,
        global_threshold_recompute_interval=_GLOBAL_INTERVAL,
        bucket_bytes=16 << 10, **kw)


def _non_exact(steps):
    """Iterations that end in a selection (not the exact global recompute),
    per bucket: with no warm-up, the counter is the step number."""
    return sum(1 for it in range(steps) if it % _GLOBAL_INTERVAL != 0)


def _snap(opt):
    return (torch.cat([b.flat_param for b in opt.buckets]).clone(),
            torch.cat([b.momentum_buf for b in opt.buckets]).clone())


def _train_cnn(sparse_step, max_grad_norm=0.0):
    from oktopk_amd.optimizer import FlatSGD
    from oktopk_amd.trainer import Trainer

    os.environ["OKTOPK_SPARSE_STEP"] = sparse_step
    try:
        torch.manual_seed(0)
        tr = Trainer("mnistnet", batch_size=8, cfg=_cfg(), dtype="fp32",
                     optimizer="flat_sgd", lr=LR, device=torch.device("cpu"))
        opt = tr.opt
        assert type(opt) is FlatSGD and len(opt.buckets) >= 2
        opt.max_grad_norm = max_grad_norm
        snaps, factors = [], []
        for _ in range(_STEPS):
            tr.step()
            tr.batches.randomize_()
            snaps.append(_snap(opt))
            if max_grad_norm:
                factors.append(float(opt.last_clip_scale))
    finally:
        os.environ.pop("OKTOPK_SPARSE_STEP", None)
    return opt, snaps, factors


@pytest.mark.parametrize("max_grad_norm", [0.0, 0.5])
def test_flat_sgd_sparse_step_on_vs_off(max_grad_norm):
    """max_grad_norm 0.5 is below every step's gradient norm here, so the
    clip engages; the CPU reference sums the sparse buckets in the dense
    order, so the factor — and with it every bit — must match."""
    opt_on, on, f_on = _train_cnn("1", max_grad_norm)
    opt_off, off, f_off = _train_cnn("0", max_grad_norm)
    assert opt_on.sparse_bucket_steps == len(opt_on.buckets) * _non_exact(_STEPS)
    assert opt_on.sparse_bucket_steps > 0 and opt_off.sparse_bucket_steps == 0
    for step, ((pa, ba), (pb, bb)) in enumerate(zip(on, off)):
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32)), step
        assert torch.equal(ba.view(torch.int32), bb.view(torch.int32)), step
    assert not torch.equal(on[0][0], on[-1][0])  # the steps did move something
    assert f_on == f_off
    if max_grad_norm:
        assert len(f_on) == _STEPS and all(f < 1.0 for f in f_on), f_on
    # the module's parameters are views of the flat storage
    p = opt_on.buckets[0].params[0]
    assert p.data_ptr() == opt_on.buckets[0].flat_param.data_ptr()


def _mlp(seed=3, width=64, layers=4):
    torch.manual_seed(seed)
    mods = []
    for _ in range(layers):
        mods += [torch.nn.Linear(width, width), torch.nn.ReLU()]
    mods.append(torch.nn.Linear(width, 8))
    return torch.nn.Sequential(*mods)


def _train_mlp(comm, rank, sparse_step, steps=_STEPS, **kw):
    from oktopk_amd.optimizer import FlatSGD

    os.environ["OKTOPK_SPARSE_STEP"] = sparse_step
    try:
        model = _mlp()
        cfg = _cfg()
        cfg.density = 0.05
        cfg.bucket_bytes = 8 << 10
        opt = FlatSGD(model.named_parameters(), comm=comm, cfg=cfg, lr=LR,
                      momentum=0.9, weight_decay=5e-4, **kw)
        assert len(opt.buckets) > 2
        for it in range(steps):
            g = torch.Generator().manual_seed(991 * rank + it)
            x = torch.randn(16, 64, generator=g)
            y = torch.randint(0, 8, (16,), generator=g)
            opt.zero_grad()
            torch.nn.functional.cross_entropy(model(x), y).backward()
            opt.step()
        opt.stop()
    finally:
        os.environ.pop("OKTOPK_SPARSE_STEP", None)
    return opt, model


def _world2(rank):
    import torch.distributed as dist

    from oktopk_amd.comm import Comm

    comm = Comm(dist.group.WORLD)
    opt_on, _ = _train_mlp(comm, rank, "1")
    assert opt_on._worker is None  # stopped; it ran on the reducer thread
    opt_off, _ = _train_mlp(comm, rank, "0")
    assert opt_on.sparse_bucket_steps == len(opt_on.buckets) * _non_exact(_STEPS)
    assert opt_off.sparse_bucket_steps == 0
    (pa, ba), (pb, bb) = _snap(opt_on), _snap(opt_off)
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
    assert torch.equal(ba.view(torch.int32), bb.view(torch.int32))
    # the ranks agree with each other
    both = [torch.empty_like(pa) for _ in range(2)]
    dist.all_gather(both, pa)
    assert torch.equal(both[0].view(torch.int32), both[1].view(torch.int32))
    both = [torch.empty_like(ba) for _ in range(2)]
    dist.all_gather(both, ba)
    assert torch.equal(both[0].view(torch.int32), both[1].view(torch.int32))


def test_flat_sgd_sparse_step_world2_reducer_thread():
    run_dist(_world2, 2)


def test_flat_sgd_all_buckets_drain_keeps_hand_over_at_world1():
    """Hooks muted during backward (graph replay, accumulation boundary):
    synchronize() reduces every bucket; at world 1 serially, sparse."""
    from oktopk_amd.optimizer import FlatSGD

    def run(sparse_step):
        os.environ["OKTOPK_SPARSE_STEP"] = sparse_step
        try:
            model = _mlp()
            cfg = _cfg()
            cfg.density, cfg.bucket_bytes = 0.05, 8 << 10
            opt = FlatSGD(model.named_parameters(), cfg=cfg, lr=LR)
            for it in range(4):
                g = torch.Generator().manual_seed(it)
                x = torch.randn(16, 64, generator=g)
                y = torch.randint(0, 8, (16,), generator=g)
                opt.zero_grad()
                opt.local = True
                torch.nn.functional.cross_entropy(model(x), y).backward()
                opt.local = False
                opt.step()
        finally:
            os.environ.pop("OKTOPK_SPARSE_STEP", None)
        return opt

    on, off = run("1"), run("0")
    assert on.sparse_bucket_steps == len(on.buckets) * _non_exact(4) > 0
    assert off.sparse_bucket_steps == 0
    for a, b in zip(_snap(on), _snap(off)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# -- optimizer surface --------------------------------------------------------

def _one_step(opt, model, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(16, 64, generator=g)
    y = torch.randint(0, 8, (16,), generator=g)
    opt.zero_grad()
    torch.nn.functional.cross_entropy(model(x), y).backward()
    opt.step()


def test_flat_sgd_lr_assignment_is_honoured_on_the_next_step():
    from oktopk_amd.optimizer import FlatSGD

    def run(lrs):
        model = _mlp()
        cfg = EngineConfig(compressor="dense", bucket_bytes=8 << 10)
        opt = FlatSGD(model.named_parameters(), cfg=cfg, lr=lrs[0], momentum=0.0)
        groups = opt.param_groups
        assert groups is opt.param_groups and len(groups) == 1
        assert set(groups[0]) == {"lr", "momentum", "weight_decay", "nesterov",
                                  "params"}
        for it, lr in enumerate(lrs):
            for g in opt.param_groups:
                g["lr"] = lr
            _one_step(opt, model, it)
        return _snap(opt)[0]

    base = run([0.1, 0.1])
    assert torch.equal(base, run([0.1, 0.1]))
    assert not torch.equal(base, run([0.1, 0.0]))
    # lr 0 on the second step: the parameters stay where the first step left
    # them
    assert torch.equal(run([0.1, 0.0]), run([0.1]))


def test_flat_sgd_state_dict_round_trip(tmp_path):
    from oktopk_amd.optimizer import FlatSGD

    def make():
        model = _mlp()
        cfg = _cfg()
        cfg.density, cfg.bucket_bytes = 0.05, 8 << 10
        return model, FlatSGD(model.named_parameters(), cfg=cfg, lr=LR,
                              momentum=0.9, weight_decay=5e-4, nesterov=True)

    model_a, a = make()
    for it in range(3):
        _one_step(a, model_a, it)
    path = tmp_path / "flat_sgd.pt"
    torch.save(a.state_dict(), path)
    model_b, b = make()
    b.param_groups[0]["lr"] = 123.0
    b.load_state_dict(torch.load(path, map_location="cpu"))
    assert b.param_groups[0]["lr"] == LR and b.param_groups[0]["nesterov"]
    for x, y in zip(_snap(a), _snap(b)):
        assert torch.equal(x, y)
    for pa, pb in zip(model_a.parameters(), model_b.parameters()):
        assert torch.equal(pa, pb)  # the module sees the loaded weights
    assert set(b.reducer.states) == set(a.reducer.states)
    # and both continue identically (residuals, thresholds, counters)
    for it in range(3, 6):
        _one_step(a, model_a, it)
        _one_step(b, model_b, it)
    for x, y in zip(_snap(a), _snap(b)):
        assert torch.equal(x, y)
    assert a.sparse_bucket_steps - b.sparse_bucket_steps == len(a.buckets) * 2


def test_flat_sgd_rejects_bf16_parameters():
    from oktopk_amd.optimizer import FlatSGD

    model = _mlp().to(torch.bfloat16)
    before = [p.data_ptr() for p in model.parameters()]
    with pytest.raises(ValueError, match="fp32"):
        FlatSGD(model.named_parameters(), lr=LR)
    assert before == [p.data_ptr() for p in model.parameters()]
    assert all(p.grad is None for p in model.parameters())


def test_trainer_and_environment_select_flat_sgd(monkeypatch):
    import oktopk_amd
    from oktopk_amd.optimizer import FlatSGD, _DistributedOptimizer
    from oktopk_amd.trainer import Trainer

    assert oktopk_amd.FlatSGD is FlatSGD
    kw = dict(batch_size=2, cfg=_cfg(), dtype="fp32", device=torch.device("cpu"))
    monkeypatch.delenv("OKTOPK_FLAT_SGD", raising=False)
    tr = Trainer("mnistnet", optimizer="flat_sgd", **kw)
    assert type(tr.opt) is FlatSGD and tr.opt_kind == "flat_sgd"
    g = tr.opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == \
        (0.1, 0.9, 5e-4, False)
    for opt_name in ("auto", "sgd"):
        tr = Trainer("mnistnet", optimizer=opt_name, **kw)
        assert type(tr.opt) is _DistributedOptimizer and tr.opt_kind == "sgd"
    monkeypatch.setenv("OKTOPK_FLAT_SGD", "1")
    for opt_name in ("auto", "sgd"):
        tr = Trainer("mnistnet", optimizer=opt_name, **kw)
        assert type(tr.opt) is FlatSGD and tr.opt_kind == "flat_sgd"
    # the step-decay schedule writes through param_groups
    tr.adjust_learning_rate(0)
    tr.adjust_learning_rate(10)  # first milestone of the non-CIFAR schedule
    assert tr.opt.param_groups[0]["lr"] == pytest.approx(0.01)


def test_train_cli_accepts_flat_sgd():
    from oktopk_amd.train import build_argparser

    args = build_argparser().parse_args(["--optimizer", "flat_sgd"])
    assert args.optimizer == "flat_sgd"
