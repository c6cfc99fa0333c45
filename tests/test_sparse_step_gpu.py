"""Sparse optimizer tail on the GPU: grad_clip_scale_sparse and the sparse
Adam kernels against the dense route on the same inputs (fill_sparse_scaled_
or zero + scatter_gt_credit_, then grad_clip_scale, then fused_adam_(mirror_)).
Adam must match to the bit — the sign of zero included; the clip scale may
differ by the order of an fp64 atomic sum only."""
import pytest
import torch

from oktopk_amd import ops

pytestmark = pytest.mark.gpu

ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6)
TILE = 1024  # elements one block covers per float4 iteration (ADAM_TILE)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


def _dense_grad(total, idx, val, scale, tau):
    t = torch.full((total,), 7.0, device="cuda")  # stale content
    if tau < 0:
        ops.fill_sparse_scaled_(t, idx, val, scale)
    else:
        t.zero_()
        ops.scatter_gt_credit_(t, torch.zeros(total, device="cuda"), idx, val,
                               tau, scale)
    return t


def _state(n, off, seed):
    """p, exp_avg, exp_avg_sq (+ bf16 mirror) of length n whose base pointers
    sit `off` elements into a 256-byte-aligned allocation; exp_avg carries
    -0.0 entries (a zero gradient must keep their sign)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n + off, generator=g).cuda()[off:]
    m = (torch.randn(n + off, generator=g) * 0.1)
    m[::3] = -0.0
    m = m.cuda()[off:]
    v = (torch.rand(n + off, generator=g) * 0.01).cuda()[off:]
    mirror = torch.zeros(n + off, dtype=torch.bfloat16, device="cuda")[off:]
    return p, m, v, mirror


def _check_adam(n, idx, val, *, base=0, total=None, scale=1.0, tau=-1.0,
                gscale=None, wd=0.01, off=0):
    """Both Adam variants (plain and mirror) over the slice [base, base+n) of
    a flat layout of `total` elements, sparse op vs dense route."""
    total = total if total is not None else base + n
    idx = idx.to(device="cuda", dtype=torch.int32)
    val = val.to(device="cuda", dtype=torch.float32)
    dense = _dense_grad(total, idx, val, scale, tau)
    # the dense route's gradient slice at the alignment of p / exp_avg /
    # exp_avg_sq, as in the optimizer's flat layout: adam_kernel picks its
    # float4 or scalar path from all four pointers, and the two paths round
    # exp_avg differently (an odd `base` alone must not flip it)
    buf = torch.empty(n + off, device="cuda")
    buf[off:].copy_(dense[base:base + n])
    gslice = buf[off:]
    for mirror_on in (False, True):
        pd, md, vd, bd = _state(n, off, 11)
        ps, ms, vs, bs = _state(n, off, 11)
        if mirror_on:
            ops.fused_adam_mirror_(pd, gslice, md, vd, bd, ADAM["lr"], ADAM["b1"],
                                   ADAM["b2"], ADAM["eps"], wd, gscale=gscale)
            ops.fused_adam_sparse_mirror_(ps, idx, val, base, scale, tau, ms, vs,
                                          bs, ADAM["lr"], ADAM["b1"], ADAM["b2"],
                                          ADAM["eps"], wd, gscale=gscale)
        else:
            ops.fused_adam_(pd, gslice, md, vd, ADAM["lr"], ADAM["b1"],
                            ADAM["b2"], ADAM["eps"], wd, gscale=gscale)
            ops.fused_adam_sparse_(ps, idx, val, base, scale, tau, ms, vs,
                                   ADAM["lr"], ADAM["b1"], ADAM["b2"],
                                   ADAM["eps"], wd, gscale=gscale)
        torch.cuda.synchronize()
        tag = f"n={n} base={base} mirror={mirror_on}"
        _same_bits(pd, ps, "p " + tag)
        _same_bits(md, ms, "exp_avg " + tag)
        _same_bits(vd, vs, "exp_avg_sq " + tag)
        _same_bits(bd, bs, "bf16 mirror " + tag)
        assert torch.equal(pd, ps) and torch.equal(md, ms)
        assert torch.equal(vd, vs) and torch.equal(bd, bs)


def _random_sel(total, m, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(total, generator=g)[:m].sort().values
    return idx, torch.randn(m, generator=g)


SIZES = [1, 3, 1023, 1024, 1025, 5000, 3 * 1024 + 2]


@pytest.mark.parametrize("n", SIZES)
def test_adam_sparse_sizes(n):
    idx, val = _random_sel(n, max(1, n // 9), n)
    _check_adam(n, idx, val)


@pytest.mark.parametrize("n", SIZES)
def test_adam_sparse_unaligned_base_pointer(n):
    """Base pointers only 4-byte aligned: both routes take the scalar path."""
    idx, val = _random_sel(n, max(1, n // 9), n + 1)
    _check_adam(n, idx, val, off=1)
    _check_adam(n, idx, val, off=3, tau=0.6)


@pytest.mark.parametrize("base,n,total", [(1000, 5000, 7000), (1001, 3 * 1024 + 2, 5000),
                                          (2048, 1024, 4096), (1016, 1, 3000)])
def test_adam_sparse_slice_at_nonzero_base(base, n, total):
    """Entries below and above the slice are ignored."""
    idx, val = _random_sel(total, total // 5, base)
    assert int(idx.min()) < base and int(idx.max()) >= base + n
    _check_adam(n, idx, val, base=base, total=total)
    _check_adam(n, idx, val, base=base, total=total, tau=0.8, scale=0.5)


def test_adam_sparse_no_entries():
    empty = torch.zeros(0, dtype=torch.int32)
    for n in (1, 1025, 5000):
        _check_adam(n, empty, torch.zeros(0))
        _check_adam(n, empty, torch.zeros(0), off=1)


def test_adam_sparse_tile_and_slice_edges():
    """Hits on the first and last element of every tile and of the slice,
    and on the elements just outside the slice."""
    base, n = 1000, 3 * TILE + 2
    total = base + n + 1000
    inside = [0, 1, 3, 4, TILE - 1, TILE, TILE + 3, 2 * TILE - 1, 2 * TILE,
              3 * TILE - 1, 3 * TILE, n - 1]
    idx = torch.tensor([0, base - 1] + [base + j for j in inside]
                       + [base + n, total - 1])
    val = torch.arange(1, idx.numel() + 1, dtype=torch.float32) * -0.37
    _check_adam(n, idx, val, base=base, total=total)
    _check_adam(n, idx, val, base=base, total=total, off=1)
    # slice starting at 0, last element a hit, n a multiple of the tile
    idx2 = torch.tensor([0, TILE - 1, TILE, 2 * TILE - 1])
    _check_adam(2 * TILE, idx2, torch.ones(4))


def test_adam_sparse_300_consecutive_in_one_tile():
    n = 5000
    idx = torch.cat([torch.tensor([5]), torch.arange(1100, 1400),
                     torch.tensor([4999])])
    g = torch.Generator().manual_seed(4)
    val = torch.randn(idx.numel(), generator=g)
    _check_adam(n, idx, val)
    _check_adam(n, idx, val, tau=0.5, off=1)


@pytest.mark.parametrize("tau", [-1.0, 0.0, 0.9])
@pytest.mark.parametrize("gs", [None, 1.0, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_sparse_tau_gscale_wd(tau, gs, wd):
    n = 3 * 1024 + 2
    idx, val = _random_sel(n, 700, 21)
    val[::11] = 0.0   # kept by tau < 0 only
    val[5::11] = -0.0
    gscale = None if gs is None else torch.tensor([gs], device="cuda")
    _check_adam(n, idx, val, tau=tau, scale=0.125 if tau < 0 else 1.0,
                gscale=gscale, wd=wd)


@pytest.mark.parametrize("tau,scale", [(-1.0, 0.5), (0.9, 1.0), (0.0, 0.125)])
@pytest.mark.parametrize("m", [0, 1, 700, 20000])
def test_grad_clip_scale_sparse(tau, scale, m):
    """The parent's fp64 sum already depends on atomic order, so the sums
    must agree within m * 2^-52 relative and the fp32 scales be equal or
    adjacent."""
    total = 50000
    idx, val = _random_sel(total, m, 31 + m)
    idx = idx.to(device="cuda", dtype=torch.int32)
    val = (val * 3.0).cuda()
    dense = _dense_grad(total, idx, val, scale, tau)
    acc_d = torch.zeros(1, dtype=torch.float64, device="cuda")
    acc_s = torch.zeros(1, dtype=torch.float64, device="cuda")
    ops.sumsq_into_(acc_d, dense)
    ops.sparse_sumsq_into_(acc_s, idx, val, scale, tau)
    sd, ss = float(acc_d), float(acc_s)
    assert abs(sd - ss) <= max(m, 1) * 2.0 ** -52 * sd, (sd, ss)
    for max_norm in (1.0, 1e9):
        gd = ops.grad_clip_scale(dense, max_norm)
        gsp = ops.grad_clip_scale_sparse(idx, val, scale, tau, max_norm, total)
        diff = int((gd.view(torch.int32) - gsp.view(torch.int32)).abs())
        assert diff <= 1, (float(gd), float(gsp))
        if max_norm == 1e9 or m == 0:
            assert float(gsp) == 1.0
        elif sd > 1.0:
            assert float(gsp) < 1.0


def test_credit_without_result():
    n = 5000
    idx, val = _random_sel(n, 600, 8)
    idx = idx.to(device="cuda", dtype=torch.int32)
    val = val.cuda()
    r_d = torch.ones(n, device="cuda")
    r_s = torch.ones(n, device="cuda")
    c_d = ops.scatter_gt_credit_(torch.zeros(n, device="cuda"), r_d, idx, val, 0.5, 1.0)
    c_s = ops.scatter_gt_credit_(None, r_s, idx, val, 0.5)
    assert c_d == c_s == int((val.abs() > 0.5).sum())
    assert torch.equal(r_d, r_s)


# -- FlatBertAdam on a small bf16 BERT, hand-over on vs off -------------------

SMALL = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2,
             intermediate_size=256, vocab_size=1000,
             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _train(monkeypatch, sparse_step, steps=6):
    from oktopk_amd.config import EngineConfig
    from oktopk_amd.trainer import Trainer

    monkeypatch.setenv("OKTOPK_SPARSE_STEP", sparse_step)
    torch.manual_seed(0)
    # exact iterations 0 and 3 fall back to the dense hand-over
    cfg = EngineConfig.preset(
        "bert", compressor="oktopk", density=0.01, dense_warmup_iters=0,
        local_threshold_recompute_interval=4,
        global_threshold_recompute_interval=3)
    tr = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg,
                 model_kwargs=SMALL, dtype="bf16")
    tr.batches.input_ids.clamp_(max=999)
    tr.batches.mlm_labels.clamp_(max=999)
    took = []
    for _ in range(steps):
        tr.step()
        took.append(tr.opt.reducer.sparse_result is not None)
    torch.cuda.synchronize()
    opt = tr.opt
    return took, (opt.flat_param.clone(), opt.flat_param_model.clone(),
                  opt.exp_avg.clone(), opt.exp_avg_sq.clone())


def test_flat_bert_adam_bf16_sparse_step_on_vs_off(monkeypatch):
    took_on, on = _train(monkeypatch, "1")
    took_off, off = _train(monkeypatch, "0")
    assert took_on == [False, True, True, False, True, True], took_on
    assert not any(took_off)
    for a, b, name in zip(on, off, ("master", "bf16 params", "exp_avg",
                                    "exp_avg_sq")):
        assert torch.equal(a, b), name
