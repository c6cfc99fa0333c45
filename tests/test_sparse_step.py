"""Sparse optimizer tail on CPU: the reference sparse clip / Adam ops against
the dense route, and FlatBertAdam with the sparse hand-over on vs off
(OKTOPK_SPARSE_STEP) — parameters and Adam state must not change by a bit,
on steps that take the hand-over and on steps that fall back alike."""
import os

import pytest
import torch

from conftest import run_dist
from oktopk_amd import ops
from oktopk_amd.config import EngineConfig
from oktopk_amd.ops import reference as ref


def _sparse_grad(n, m, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(n, generator=g)[:m].sort().values.to(torch.int32)
    val = torch.randn(m, generator=g)
    return idx, val


def _dense(idx, val, n, scale, tau):
    """The dense route's gradient: fill_sparse_scaled_ (tau < 0) or zero +
    scatter_gt_credit_."""
    t = torch.full((n,), 7.0)  # stale content must not survive
    if tau < 0:
        ops.fill_sparse_scaled_(t, idx, val, scale)
    else:
        t.zero_()
        ops.scatter_gt_credit_(t, torch.zeros(n), idx, val, tau, scale)
    return t


@pytest.mark.parametrize("tau,scale", [(-1.0, 0.5), (0.7, 1.0), (0.0, 0.25)])
def test_reference_sparse_ops_match_dense_route(tau, scale):
    n, m = 5000, 400
    idx, val = _sparse_grad(n, m, 3)
    g = _dense(idx, val, n, scale, tau)
    assert torch.equal(ref.densify_sparse_grad(idx, val, 0, n, scale, tau), g)

    gs_d = ops.grad_clip_scale(g, 1.0)
    gs_s = ops.grad_clip_scale_sparse(idx, val, scale, tau, 1.0, n)
    assert torch.equal(gs_d, gs_s) and float(gs_s) < 1.0
    # a norm under the bound clips nothing
    assert float(ops.grad_clip_scale_sparse(idx, val, scale, tau, 1e6, n)) == 1.0

    gen = torch.Generator().manual_seed(5)
    for base, ln, wd in [(0, n, 0.01), (1234, 2000, 0.0), (4000, 1000, 0.01)]:
        p0 = torch.randn(ln, generator=gen)
        m0 = torch.randn(ln, generator=gen) * 0.1
        m0[::7] = -0.0
        v0 = torch.rand(ln, generator=gen) * 0.01
        pd, md, vd = p0.clone(), m0.clone(), v0.clone()
        ps, ms, vs = p0.clone(), m0.clone(), v0.clone()
        ops.fused_adam_(pd, g[base:base + ln].clone(), md, vd, 1e-3, 0.9,
                        0.999, 1e-6, wd, gscale=gs_d)
        ops.fused_adam_sparse_(ps, idx, val, base, scale, tau, ms, vs, 1e-3,
                               0.9, 0.999, 1e-6, wd, gscale=gs_s)
        assert torch.equal(pd, ps) and torch.equal(md, ms) and torch.equal(vd, vs)
        assert torch.equal(torch.signbit(md), torch.signbit(ms))


def test_reference_sparse_mirror_and_credit():
    n, m = 1025, 90
    idx, val = _sparse_grad(n, m, 9)
    g = _dense(idx, val, n, 1.0, 0.5)
    p0, m0, v0 = torch.randn(n), torch.zeros(n), torch.zeros(n)
    pd, md, vd, bd = p0.clone(), m0.clone(), v0.clone(), torch.zeros(n, dtype=torch.bfloat16)
    ps, ms, vs, bs = p0.clone(), m0.clone(), v0.clone(), torch.zeros(n, dtype=torch.bfloat16)
    ops.fused_adam_mirror_(pd, g, md, vd, bd, 1e-3, 0.9, 0.999, 1e-6, 0.01)
    ops.fused_adam_sparse_mirror_(ps, idx, val, 0, 1.0, 0.5, ms, vs, bs,
                                  1e-3, 0.9, 0.999, 1e-6, 0.01)
    assert torch.equal(pd, ps) and torch.equal(bd, bs)
    assert torch.equal(md, ms) and torch.equal(vd, vs)

    # credit without a result: same residual, same count as the dense op
    r_d, r_s = torch.ones(n), torch.ones(n)
    c_d = ops.scatter_gt_credit_(torch.zeros(n), r_d, idx, val, 0.5, 1.0)
    c_s = ops.scatter_gt_credit_(None, r_s, idx, val, 0.5)
    assert c_d == c_s == int((val.abs() > 0.5).sum())
    assert torch.equal(r_d, r_s)


# -- FlatBertAdam, hand-over on vs off ---------------------------------------

_TINY = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=2,
             intermediate_size=128)
_STEPS = 6


def _train(comm, sparse_step):
    """6 steps of a tiny BERT; recompute intervals chosen so the run has
    exact iterations (0 and 3: dense fall-back) and non-exact ones (1, 2, 4,
    5: hand-over), and a local-threshold recompute (4) in between."""
    from oktopk_amd.trainer import Trainer

    os.environ["OKTOPK_SPARSE_STEP"] = sparse_step
    try:
        torch.manual_seed(0)
        cfg = EngineConfig.preset(
            "bert", compressor="oktopk", density=0.01, dense_warmup_iters=0,
            local_threshold_recompute_interval=4,
            global_threshold_recompute_interval=3)
        tr = Trainer("bert_base", batch_size=2, seq_len=16, comm=comm, cfg=cfg,
                     dtype="fp32", model_kwargs=_TINY)
        took = []
        for _ in range(_STEPS):
            tr.step()
            took.append(tr.opt.reducer.sparse_result is not None)
    finally:
        os.environ.pop("OKTOPK_SPARSE_STEP", None)
    opt = tr.opt
    return took, (opt.flat_param.clone(), opt.exp_avg.clone(),
                  opt.exp_avg_sq.clone(),
                  opt.reducer.states["flat"].residual.clone())


def _assert_same_training(comm):
    took_on, on = _train(comm, "1")
    took_off, off = _train(comm, "0")
    assert took_on == [False, True, True, False, True, True], took_on
    assert not any(took_off)
    for a, b, name in zip(on, off, ("param", "exp_avg", "exp_avg_sq", "residual")):
        assert torch.equal(a, b), name
    assert float(on[1].abs().max()) > 0.0  # the steps did move something


def test_flat_adam_sparse_step_world1():
    _assert_same_training(None)


def _world2(rank):
    import torch.distributed as dist

    from oktopk_amd.comm import Comm

    _assert_same_training(Comm(dist.group.WORLD))


def test_flat_adam_sparse_step_world2():
    run_dist(_world2, 2)
