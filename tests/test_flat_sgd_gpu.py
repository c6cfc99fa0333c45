"""Flat SGD on the GPU.  sgd_step_ must equal the reference composition of
separate torch mul / add calls run on the same device, to the bit (float4
loop and scalar tail alike); sgd_step_sparse_ must equal fill_sparse_scaled_
(or zero + scatter_gt_credit_) followed by sgd_step_, to the bit — the sign
of zero included.  The clip factor may differ by the order of an fp64 atomic
sum only.  FlatSGD under the Trainer: sparse hand-over on vs off."""
import pytest
import torch

from oktopk_amd import ops
from oktopk_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

LR = 0.05
TILE = 1024  # elements one block covers per float4 iteration (ADAM_TILE)
# 1 .. 3*1024+2: tail only, one float4 + tail, tile edges, several blocks;
# the last: n_blocks(n, 8) = 1025 blocks over 2050 float4 tiles, so blocks
# run a second grid-stride tile while the last tile is partial and a scalar
# tail of 3 follows
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 5000, 3 * 1024 + 2,
         2048 * 1024 + 1024 + 3]


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


def _state(n, off, seed):
    """p and buf of length n whose base pointers sit `off` elements into an
    aligned allocation; buf carries -0.0 entries."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n + off, generator=g).cuda()[off:]
    buf = torch.randn(n + off, generator=g) * 0.1
    buf[::3] = -0.0
    return p, buf.cuda()[off:]


def _dense_grad(total, idx, val, scale, tau):
    t = torch.full((total,), 7.0, device="cuda")  # stale content
    if tau < 0:
        ops.fill_sparse_scaled_(t, idx, val, scale)
    else:
        t.zero_()
        ops.scatter_gt_credit_(t, torch.zeros(total, device="cuda"), idx, val,
                               tau, scale)
    return t


def _random_sel(total, m, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(total, generator=g)[:m].sort().values
    return idx, torch.randn(m, generator=g)


def _check(n, idx, val, *, base=0, total=None, scale=1.0, tau=-1.0, gscale=None,
           momentum=0.9, nesterov=False, wd=5e-4, off=0):
    """Over the slice [base, base+n) of a flat layout of `total` elements:
    the reference composition == sgd_step_ == sgd_step_sparse_, bit for bit."""
    total = total if total is not None else base + n
    idx = idx.to(device="cuda", dtype=torch.int32)
    val = val.to(device="cuda", dtype=torch.float32)
    dense = _dense_grad(total, idx, val, scale, tau)
    # the gradient slice at the alignment of p / buf, as in a flat layout
    gbuf = torch.empty(n + off, device="cuda")
    gbuf[off:].copy_(dense[base:base + n])
    gslice = gbuf[off:]
    pr, br = _state(n, off, 11)
    pd, bd = _state(n, off, 11)
    ps, bs = _state(n, off, 11)
    p0, b0 = _state(n, off, 11)
    ref.sgd_step_(pr, gslice, br, LR, momentum, wd, nesterov, gscale)
    ops.sgd_step_(pd, gslice, bd, LR, momentum, wd, nesterov, gscale=gscale)
    ops.sgd_step_sparse_(ps, idx, val, base, scale, tau, bs, LR, momentum, wd,
                         nesterov, gscale=gscale)
    torch.cuda.synchronize()
    tag = f"n={n} base={base} off={off} mom={momentum} nest={nesterov} wd={wd}"
    _same_bits(pr, pd, "p reference vs dense " + tag)
    _same_bits(br, bd, "buf reference vs dense " + tag)
    _same_bits(pd, ps, "p dense vs sparse " + tag)
    _same_bits(bd, bs, "buf dense vs sparse " + tag)
    if momentum == 0:
        _same_bits(bd, b0, "buf touched without momentum " + tag)
    if n > 16:
        assert not torch.equal(pd, p0), "nothing moved " + tag


@pytest.mark.parametrize("n", SIZES)
def test_sgd_step_sizes(n):
    idx, val = _random_sel(n, max(1, n // 9) if n < 10**6 else n // 1000, n)
    _check(n, idx, val)
    if n < 10**6:
        _check(n, idx, val, nesterov=True, tau=0.6,
               gscale=torch.tensor([0.37], device="cuda"))


@pytest.mark.parametrize("n", SIZES[:-1])
def test_sgd_step_unaligned_base_pointer(n):
    """Base pointers only 4-byte aligned: all routes take the scalar path."""
    idx, val = _random_sel(n, max(1, n // 9), n + 1)
    _check(n, idx, val, off=1)
    _check(n, idx, val, off=3, tau=0.6, nesterov=True)


@pytest.mark.parametrize("base,n,total", [(1000, 5000, 7000), (1001, 3 * 1024 + 2, 5000),
                                          (2048, 1024, 4096), (1016, 1, 3000)])
def test_sgd_step_sparse_slice_at_nonzero_base(base, n, total):
    """Entries below and above the slice are ignored."""
    idx, val = _random_sel(total, total // 5, base)
    assert int(idx.min()) < base and int(idx.max()) >= base + n
    _check(n, idx, val, base=base, total=total)
    _check(n, idx, val, base=base, total=total, tau=0.8, scale=0.5, off=1)


def test_sgd_step_sparse_no_entries():
    empty = torch.zeros(0, dtype=torch.int32)
    for n in (1, 1025, 5000):
        _check(n, empty, torch.zeros(0))
        _check(n, empty, torch.zeros(0), off=1, nesterov=True)


def test_sgd_step_sparse_tile_and_slice_edges():
    """Hits on the first and last element of every tile and of the slice,
    and on the elements just outside the slice."""
    base, n = 1000, 3 * TILE + 2
    total = base + n + 1000
    inside = [0, 1, 3, 4, TILE - 1, TILE, TILE + 3, 2 * TILE - 1, 2 * TILE,
              3 * TILE - 1, 3 * TILE, n - 1]
    idx = torch.tensor([0, base - 1] + [base + j for j in inside]
                       + [base + n, total - 1])
    val = torch.arange(1, idx.numel() + 1, dtype=torch.float32) * -0.37
    _check(n, idx, val, base=base, total=total)
    _check(n, idx, val, base=base, total=total, off=1)
    # slice starting at 0, last element a hit, n a multiple of the tile
    idx2 = torch.tensor([0, TILE - 1, TILE, 2 * TILE - 1])
    _check(2 * TILE, idx2, torch.ones(4))


def test_sgd_step_sparse_300_consecutive_in_one_tile():
    n = 5000
    idx = torch.cat([torch.tensor([5]), torch.arange(1100, 1400),
                     torch.tensor([4999])])
    g = torch.Generator().manual_seed(4)
    val = torch.randn(idx.numel(), generator=g)
    _check(n, idx, val)
    _check(n, idx, val, tau=0.5, off=1)


@pytest.mark.parametrize("tau", [-1.0, 0.0, 0.9])
@pytest.mark.parametrize("gs", [None, 0.37])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_step_grid(momentum, nesterov, wd, gs, tau):
    n = 3 * 1024 + 2
    idx, val = _random_sel(n, 700, 21)
    val[::11] = 0.0   # kept by tau < 0 only
    val[5::11] = -0.0
    gscale = None if gs is None else torch.tensor([gs], device="cuda")
    _check(n, idx, val, tau=tau, scale=0.125 if tau < 0 else 1.0,
           gscale=gscale, momentum=momentum, nesterov=nesterov, wd=wd)


@pytest.mark.parametrize("n", [5, 3 * 1024 + 2])
def test_sgd_step_momentum_zero_with_an_empty_buffer(n):
    idx, val = _random_sel(n, max(1, n // 9), 5)
    idx = idx.to(device="cuda", dtype=torch.int32)
    val = val.cuda()
    g = _dense_grad(n, idx, val, 1.0, -1.0)
    empty = torch.zeros(0, device="cuda")
    for nesterov in (False, True):
        pr, _ = _state(n, 0, 3)
        pd, _ = _state(n, 0, 3)
        ps, _ = _state(n, 0, 3)
        ref.sgd_step_(pr, g, empty, LR, 0.0, 5e-4, nesterov)
        ops.sgd_step_(pd, g, empty, LR, 0.0, 5e-4, nesterov)
        ops.sgd_step_sparse_(ps, idx, val, 0, 1.0, -1.0, empty, LR, 0.0, 5e-4,
                             nesterov)
        torch.cuda.synchronize()
        _same_bits(pr, pd, "reference vs dense")
        _same_bits(pd, ps, "dense vs sparse")


def test_sgd_step_rejects_a_short_buffer():
    p, buf = _state(100, 0, 1)
    with pytest.raises(RuntimeError):
        ops.sgd_step_(p, torch.zeros(100, device="cuda"), buf[:50], LR, 0.9,
                      0.0, False)
    with pytest.raises(RuntimeError):
        ops.sgd_step_(p, torch.zeros(99, device="cuda"), buf, LR, 0.9, 0.0,
                      False)


@pytest.mark.parametrize("tau,scale", [(-1.0, 0.5), (0.9, 1.0)])
def test_clip_across_sparse_and_dense_buckets(tau, scale):
    """Three buckets into ONE accumulator, the middle one dense in both
    routes, the others sparse in one route.  The fp64 sum already depends on
    atomic order, so the sums must agree within m * 2^-52 relative and the
    fp32 factors be equal or adjacent (test_grad_clip_scale_sparse's
    criterion)."""
    sizes, ms = [50000, 5000, 3 * 1024 + 2], [700, 0, 90]
    acc_d = torch.zeros(1, dtype=torch.float64, device="cuda")
    acc_s = torch.zeros(1, dtype=torch.float64, device="cuda")
    m_total = 0
    for j, (n, m) in enumerate(zip(sizes, ms)):
        if m == 0:
            g = torch.randn(n, generator=torch.Generator().manual_seed(j)).cuda()
            ops.sumsq_into_(acc_d, g)
            ops.sumsq_into_(acc_s, g)
            continue
        idx, val = _random_sel(n, m, 40 + j)
        idx = idx.to(device="cuda", dtype=torch.int32)
        val = (val * 3.0).cuda()
        ops.sumsq_into_(acc_d, _dense_grad(n, idx, val, scale, tau))
        ops.sparse_sumsq_into_(acc_s, idx, val, scale, tau, n=n)
        m_total += m
    sd, ss = float(acc_d), float(acc_s)
    # the dense bucket's 5000 terms are summed by the same kernel in both
    assert abs(sd - ss) <= (m_total + sizes[1]) * 2.0 ** -52 * sd, (sd, ss)
    for max_norm in (1.0, 1e9):
        fd = ops.clip_scale_from_sumsq(acc_d, max_norm)
        fs = ops.clip_scale_from_sumsq(acc_s, max_norm)
        assert fd.dtype == torch.float32 and fd.is_cuda
        diff = int((fd.view(torch.int32) - fs.view(torch.int32)).abs())
        assert diff <= 1, (float(fd), float(fs))
        # the HIP factor is the reference formula on the same sum
        assert float(fd) == float(ref.clip_scale_from_sumsq(acc_d.cpu(), max_norm))
        if max_norm == 1e9:
            assert float(fs) == 1.0
        else:
            assert sd > 1.0 and float(fs) < 1.0


# -- FlatSGD under the Trainer: resnet20, graph capture after 2 steps ---------

_STEPS = 6
_GLOBAL_INTERVAL = 3


def _train(monkeypatch, sparse_step):
    from oktopk_amd.config import EngineConfig
    from oktopk_amd.optimizer import FlatSGD
    from oktopk_amd.trainer import Trainer

    monkeypatch.setenv("OKTOPK_SPARSE_STEP", sparse_step)
    # The two runs must differ by the optimizer route alone, so the model
    # arithmetic has to be reproducible run to run: fp32 and deterministic
    # convolutions.  (Under bf16 autocast the convolution backward is not —
    # two runs of the SAME route already differ in the raw gradient of step
    # 0.)  With benchmark off (the Trainer turns it on) the convolutions take
    # MIOpen's immediate mode, which spares the test the ~20 s solver search
    # of the first step.
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    torch.manual_seed(0)
    cfg = EngineConfig.preset(
        "vgg", compressor="oktopk", density=0.01, dense_warmup_iters=0,
        local_threshold_recompute_interval=4,
        global_threshold_recompute_interval=_GLOBAL_INTERVAL,
        bucket_bytes=256 << 10)
    tr = Trainer("resnet20", batch_size=8, cfg=cfg, optimizer="flat_sgd",
                 lr=LR, dtype="fp32")
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    opt = tr.opt
    assert type(opt) is FlatSGD and len(opt.buckets) >= 2
    took, captured = [], None
    for it in range(_STEPS):
        if it == 2:
            captured = tr.capture_graph()
        before = opt.sparse_bucket_steps
        tr.step()
        took.append(opt.sparse_bucket_steps - before)
    torch.cuda.synchronize()
    return (captured, len(opt.buckets), took,
            torch.cat([b.flat_param for b in opt.buckets]).clone(),
            torch.cat([b.momentum_buf for b in opt.buckets]).clone())


def test_flat_sgd_trainer_sparse_step_on_vs_off(monkeypatch):
    cap_on, nb, took_on, p_on, b_on = _train(monkeypatch, "1")
    cap_off, _, took_off, p_off, b_off = _train(monkeypatch, "0")
    assert cap_on and cap_off, "resnet20 fwd+bwd must capture"
    # every bucket takes the sparse route on every non-exact step: eager
    # steps from the hooks, replayed steps from the all-buckets drain
    want = [0 if it % _GLOBAL_INTERVAL == 0 else nb for it in range(_STEPS)]
    assert took_on == want, took_on
    assert not any(took_off)
    _same_bits(p_on, p_off, "parameters")
    _same_bits(b_on, b_off, "momentum")
    assert bool(torch.isfinite(p_on).all()) and float(b_on.abs().max()) > 0.0
