"""HIP gaussian_select_ef (ops/csrc/gauss_select.hip) against the torch oracle,
plus the engine with gaussian_device_select on the GPU.

Tolerances: mean/std are fp64 on both sides and differ only in summation
order (rtol 1e-12 on std, atol 1e-12*max(|mean|, std) on mean); tau0 is one
fp32 rounding (<= 6e-8) of an fp64 value (rtol 1e-6); everything downstream
of the device's own tau0 is exact."""
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import run_dist

from oktopk_amd import ops
from oktopk_amd.ops import reference as R

from test_gauss_select import CASE_TABLE, case_inputs

SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 8191,
         65537, 4_196_358]
DENSITIES = [0.05, 0.001]


def _k(n, density):
    return max(1, int(n * density))


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _bits(x):
    return x.contiguous().view(torch.int32)


_inputs = {}


def _randn_case(n):
    """(t, residual) on the CPU, generated once per size."""
    if n not in _inputs:
        g = torch.Generator().manual_seed(n)
        _inputs[n] = (torch.randn(n, generator=g),
                      torch.randn(n, generator=g) * 0.1)
    return _inputs[n]


def _replay(restored, tau0, k):
    """The host refine loop on the restored tensor from the device's tau0."""
    tau, factor = float(tau0), 1.0
    for _ in range(3):
        cnt = R.count_gt(restored, tau)
        if cnt < 2 * k / 3:
            tau *= 0.5
            factor *= 0.5
        elif cnt > 4 * k / 3:
            tau *= 1.5
            factor *= 1.5
        else:
            break
    return factor


def _check(t, res, grad, density):
    """Run the HIP op on GPU copies and check it against the oracle and
    against exact replays from its own tau0.  Returns the device outputs."""
    n = t.numel()
    k = _k(n, density)
    restored = (grad.float() if grad is not None else t) + res
    o_res = res.clone()
    _, _, _, _, _, o_tau0, o_mean, o_std = R.gaussian_select_ef(
        t, o_res, grad, density, k)

    dt, dres = t.cuda(), res.cuda()
    dgrad = grad.cuda() if grad is not None else None
    idx, val, chosen, count, tau, tau0, mean, std = ops.gaussian_select_ef(
        dt, dres, dgrad, density, k)
    print(f"n={n} d={density} mean={mean!r}/{o_mean!r} std={std!r}/{o_std!r} "
          f"tau0={tau0!r}/{o_tau0!r} chosen={chosen} count={count}")

    assert abs(std - o_std) <= 1e-12 * abs(o_std)
    assert abs(mean - o_mean) <= 1e-12 * max(abs(o_mean), o_std)
    assert abs(tau0 - o_tau0) <= 1e-6 * abs(o_tau0)
    assert tau0 == _f32(tau0)
    assert tau == _f32(tau0 * R.GAUSS_FACTORS[chosen])

    # exactness given the device's own tau0
    assert R.GAUSS_FACTORS[chosen] == _replay(restored, tau0, k)
    gi, gv = R.compact_gt(restored, tau)
    assert torch.equal(idx.cpu(), gi)
    assert torch.equal(_bits(val.cpu()), _bits(gv))
    assert count == idx.numel()
    assert torch.equal(_bits(dres.cpu()), _bits(restored))
    assert torch.equal(_bits(dt.cpu()), _bits(t))
    return idx, val, chosen, count, tau, tau0, mean, std


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("n", SIZES)
def test_randn(n, density):
    t, res = _randn_case(n)
    _check(t, res, None, density)


@pytest.mark.parametrize("case,density,factor", CASE_TABLE)
def test_case_table(case, density, factor):
    v = case_inputs()[case]
    out = _check(v, torch.zeros_like(v), None, density)
    assert R.GAUSS_FACTORS[out[2]] == factor


@pytest.mark.parametrize("n", [1, 513, 8191, 65537])
def test_bf16_grad(n):
    t, res = _randn_case(n)
    grad = t.bfloat16()
    stale = torch.full((n,), 7.0)  # t must be neither read nor written
    _check(stale, res, grad, 0.05)


def _same(a, b):
    assert torch.equal(a[0], b[0])
    assert torch.equal(_bits(a[1]), _bits(b[1]))
    assert a[2:] == b[2:]


@pytest.mark.parametrize("with_grad", [False, True])
@pytest.mark.parametrize("n", [9, 2049, 65537])
def test_misaligned_views(n, with_grad):
    """buf[1:] views (4-byte / 2-byte alignment only) take the scalar
    kernels and give the answers of the aligned copies."""
    t, res = _randn_case(n)
    k = _k(n, 0.05)
    grad = t.bfloat16() if with_grad else None

    def off(x):
        buf = torch.empty(n + 1, dtype=x.dtype, device="cuda")
        buf[1:].copy_(x)
        v = buf[1:]
        assert v.data_ptr() % 16 != 0
        return v

    at, ares = t.cuda(), res.cuda()
    ag = grad.cuda() if with_grad else None
    mt, mres = off(t), off(res)
    mg = off(grad) if with_grad else None
    a = ops.gaussian_select_ef(at, ares, ag, 0.05, k)
    m = ops.gaussian_select_ef(mt, mres, mg, 0.05, k)
    _same(a, m)
    assert torch.equal(_bits(ares), _bits(mres))
    assert torch.equal(_bits(mt), _bits(at))


@pytest.mark.parametrize("n", [65537, 4_196_358])
def test_repeatable(n):
    t, res = _randn_case(n)
    dt = t.cuda()
    a = ops.gaussian_select_ef(dt, res.cuda(), None, 0.001, _k(n, 0.001))
    b = ops.gaussian_select_ef(dt, res.cuda(), None, 0.001, _k(n, 0.001))
    _same(a, b)


def test_degenerate():
    # constant: tau0 == |c|, nothing selected, residual == restored
    t = torch.full((1000,), 1.5).cuda()
    res = torch.full((1000,), -4.0).cuda()
    idx, val, chosen, count, tau, tau0, mean, std = ops.gaussian_select_ef(
        t, res, None, 0.01, 10)
    assert (tau0, mean, std) == (2.5, -2.5, 0.0)
    assert R.GAUSS_FACTORS[chosen] == 1.125 and count == 0 == idx.numel()
    assert bool((res == -2.5).all()) and bool((t == 1.5).all())
    # all zeros
    z = torch.zeros(300).cuda()
    out = ops.gaussian_select_ef(z, torch.zeros(300).cuda(), None, 0.01, 3)
    assert out[3] == 0 and out[4] == 0.0 and out[5] == 0.0
    assert R.GAUSS_FACTORS[out[2]] == 0.125


def test_argument_checks():
    t = torch.zeros(8).cuda()
    r = torch.zeros(8).cuda()
    for density, k in ((0.0, 1), (1.5, 1), (0.1, 0)):
        with pytest.raises(RuntimeError):
            ops.gaussian_select_ef(t, r, None, density, k)
    with pytest.raises(RuntimeError):
        ops.gaussian_select_ef(t, torch.zeros(9).cuda(), None, 0.1, 1)
    with pytest.raises(RuntimeError):
        ops.gaussian_select_ef(t[:0], r[:0], None, 0.1, 1)


# -- engine on the GPU ----------------------------------------------------------

N = 200_000
DENSITY = 0.01
COMPS = ("gaussiank", "gaussiankconcat", "gaussiankSA")


def _grad(rank, it):
    g = torch.Generator().manual_seed(1000 * rank + it)
    return torch.randn(N, generator=g)


def _engine_gpu(rank):
    import torch.distributed as dist

    from oktopk_amd import AllReducer, Comm, EngineConfig
    from oktopk_amd.config import OkTopkConfig

    torch.cuda.set_device(0)
    world = dist.get_world_size()
    calls = [0]
    orig = ops.count_gt

    def counting(*a, **kw):
        calls[0] += 1
        return orig(*a, **kw)

    ops.count_gt = counting

    def build(comp):
        return AllReducer(
            Comm(dist.group.WORLD),
            EngineConfig(compressor=comp, density=DENSITY,
                         gaussian_device_select=True,
                         oktopk=OkTopkConfig(dense_warmup_iters=1)))

    for comp in COMPS:
        eng, eng16 = build(comp), build(comp)
        in_sum = torch.zeros(N, device="cuda")
        out_sum = torch.zeros(N, device="cuda")
        for it in range(5):
            # bf16-representable inputs so the grad_src twin sees the same
            g16 = _grad(rank, it).bfloat16().cuda()
            t = g16.float()
            in_sum += t
            before = calls[0]
            out = eng.run("w", t.clone())
            if it >= 1:  # steady state: no per-round host sync
                assert calls[0] == before, (comp, it)
            out_sum += out
            assert out.is_cuda and torch.isfinite(out).all()
            # identical on every rank
            ref = out.cpu()
            dist.broadcast(ref, src=0)
            assert torch.equal(out.cpu(), ref), (comp, it)
            # bf16 grad_src == caller upcasts first
            o16 = eng16.run("w", torch.full((N,), 9.0, device="cuda"),
                            grad_src=g16)
            assert torch.equal(o16, out), (comp, it)
        assert 0 < int((out != 0).sum()) < N // 2
        res = eng.states["w"].residual.clone()
        assert torch.equal(res, eng16.states["w"].residual)
        for x in (in_sum, res):
            xc = x.cpu()
            dist.all_reduce(xc)
            x.copy_(xc.cuda())
        err = (world * out_sum + res - in_sum).abs().max().item()
        assert err < 1e-2, f"{comp}: EF mass leak {err} (GPU world-{world})"
    assert calls[0] == 0


def test_engine_gpu_world1():
    run_dist(_engine_gpu, 1)


def test_engine_gpu_world2():
    run_dist(_engine_gpu, 2)
