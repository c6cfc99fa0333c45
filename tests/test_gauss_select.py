"""Device-resident Gaussian-k selection: the torch oracle
(ops.reference.gaussian_select_ef) against today's host path, branch coverage
of the refine tree, degenerate inputs, and the engine with
EngineConfig.gaussian_device_select on (gloo worlds 1/2/4 on CPU)."""
import os

import pytest
import torch

from conftest import run_dist

from oktopk_amd.ops import reference as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "gauss_flag_off_world2.pt")


def _k(n, density):
    return max(1, int(n * density))


def _host_loop(v, tau0, k):
    """The refine loop of AllReducer._gaussiank, started from tau0; returns
    the factor it ends on."""
    tau, factor = float(tau0), 1.0
    for _ in range(3):
        cnt = R.count_gt(v, tau)
        if cnt < 2 * k / 3:
            tau *= 0.5
            factor *= 0.5
        elif cnt > 4 * k / 3:
            tau *= 1.5
            factor *= 1.5
        else:
            break
    return factor


def case_inputs(n=8191, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    u = torch.rand(n, generator=g) * 2 - 1
    sparse = torch.zeros(n)
    sparse[::1000] = x[::1000]
    return {"normal": x, "x^5": x ** 5, "uniform": u, "cubed": x ** 3,
            "shifted": x + 1000, "sparse": sparse}


# (case, density, factor the reference loop ends on)
CASE_TABLE = [
    ("normal", 0.01, 1.0),
    ("x^5", 0.01, 1.5),
    ("x^5", 0.05, 0.5),
    ("uniform", 0.01, 0.375),
    ("cubed", 0.01, 1.125),
    ("shifted", 0.01, 1.125),
    ("sparse", 0.01, 0.125),
    ("cubed", 0.001, 3.375),
]


# -- oracle vs the host path --------------------------------------------------

@pytest.mark.parametrize("density", [0.05, 0.01, 0.001])
def test_oracle_matches_host_threshold(density):
    from oktopk_amd.allreducer import _gaussian_threshold

    n = 65537
    v = torch.randn(n, generator=torch.Generator().manual_seed(0))
    k = _k(n, density)
    res = torch.zeros(n)
    t0 = v.clone()
    idx, val, chosen, count, tau, tau0, mean, std = R.gaussian_select_ef(
        v, res, None, density, k)
    assert torch.equal(v, t0)          # t untouched
    assert torch.equal(res, v)         # snapshot written
    host = _gaussian_threshold(v, density)
    assert abs(tau0 - host) <= 1e-5 * host, (tau0, host)
    assert R.GAUSS_FACTORS[chosen] == _host_loop(v, tau0, k)
    gi, gv = R.compact_gt(v, tau)
    assert torch.equal(idx, gi) and torch.equal(val, gv)
    assert count == idx.numel()
    assert tau == R.gaussian_candidates(tau0)[chosen]


def test_bf16_grad_restore():
    n = 4099
    g = torch.Generator().manual_seed(3)
    grad = torch.randn(n, generator=g).bfloat16()
    res = torch.randn(n, generator=g) * 0.1
    restored = grad.float() + res
    t = torch.full((n,), 7.0)
    r1 = res.clone()
    a = R.gaussian_select_ef(t, r1, grad, 0.01, _k(n, 0.01))
    r2 = res.clone()
    b = R.gaussian_select_ef(grad.float(), r2, None, 0.01, _k(n, 0.01))
    assert torch.equal(r1, restored) and torch.equal(r2, restored)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2:] == b[2:]
    assert bool((t == 7.0).all())


# -- refine-tree branch coverage ----------------------------------------------

@pytest.mark.parametrize("case,density,factor", CASE_TABLE)
def test_tree_case(case, density, factor):
    v = case_inputs()[case]
    n = v.numel()
    k = _k(n, density)
    res = torch.zeros(n)
    idx, val, chosen, count, tau, tau0, mean, std = R.gaussian_select_ef(
        v, res, None, density, k)
    assert _host_loop(v, tau0, k) == factor, (case, density)
    assert R.GAUSS_FACTORS[chosen] == factor, (case, density, chosen)
    assert count == R.count_gt(v, tau) == idx.numel()


def test_case_table_covers_seven_factors():
    assert {f for _, _, f in CASE_TABLE} >= {
        1.0, 1.5, 0.5, 0.375, 1.125, 0.125, 3.375}


def test_tree_walk_indices():
    """Every (low/high)^3 move sequence lands on the candidate whose factor
    is the product of the moves."""
    import itertools

    k = 300
    lo, hi, ok = 0, 10 ** 6, k  # counts that force low / high / stop
    for moves in itertools.product("LH", repeat=3):
        counts = [ok] * 10
        l = h = 0
        factor = 1.0
        for m in moves:
            counts[l * (l + 1) // 2 + h] = lo if m == "L" else hi
            l += 1
            h += m == "H"
            factor *= 0.5 if m == "L" else 1.5
        j = R.gaussian_tree_walk(counts, k)
        assert R.GAUSS_FACTORS[j] == factor, moves
    # boundary: 3*cnt == 2k and 3*cnt == 4k both stop
    assert R.gaussian_tree_walk([200] + [0] * 9, 300) == 0
    assert R.gaussian_tree_walk([400] + [0] * 9, 300) == 0
    assert R.gaussian_tree_walk([199] + [300] * 9, 300) == 1
    assert R.gaussian_tree_walk([401] + [300] * 9, 300) == 2


# -- degenerate inputs ----------------------------------------------------------

def test_constant_tensor():
    n, c = 1000, -2.5
    t = torch.full((n,), 1.5)
    res = torch.full((n,), -4.0)
    idx, val, chosen, count, tau, tau0, mean, std = R.gaussian_select_ef(
        t, res, None, 0.01, 10)
    assert tau0 == abs(c) and std == 0.0 and mean == c
    # nothing is strictly above |c|: low (everything), high (everything),
    # high -> 1.125 |c| selects nothing; EF defers the whole tensor
    assert R.GAUSS_FACTORS[chosen] == 1.125
    assert count == 0 and idx.numel() == 0 and val.numel() == 0
    assert torch.equal(res, torch.full((n,), c))
    assert bool((t == 1.5).all())


def test_n1():
    t = torch.tensor([0.75])
    res = torch.tensor([0.25])
    idx, val, chosen, count, tau, tau0, mean, std = R.gaussian_select_ef(
        t, res, None, 0.01, 1)
    assert tau0 == 1.0 and mean == 1.0 and std == 0.0
    assert R.GAUSS_FACTORS[chosen] == 0.5 and count == 1
    assert idx.tolist() == [0] and val.tolist() == [1.0]
    assert res.tolist() == [1.0] and t.tolist() == [0.75]


def test_all_zeros():
    t = torch.zeros(300)
    res = torch.zeros(300)
    idx, val, chosen, count, tau, tau0, mean, std = R.gaussian_select_ef(
        t, res, None, 0.01, 3)
    assert tau0 == 0.0 and tau == 0.0 and count == 0 and idx.numel() == 0
    assert R.GAUSS_FACTORS[chosen] == 0.125
    assert not res.any()


def test_argument_checks():
    t = torch.zeros(4)
    with pytest.raises(ValueError):
        R.gaussian_select_ef(t, torch.zeros(4), None, 0.0, 1)
    with pytest.raises(ValueError):
        R.gaussian_select_ef(t, torch.zeros(4), None, 1.5, 1)
    with pytest.raises(ValueError):
        R.gaussian_select_ef(t, torch.zeros(4), None, 0.1, 0)
    with pytest.raises(ValueError):
        R.gaussian_select_ef(t, torch.zeros(5), None, 0.1, 1)


# -- engine ---------------------------------------------------------------------

N = 8192
DENSITY = 0.02
ITERS = 8
COMPS = ("gaussiank", "gaussiankconcat", "gaussiankSA")


def _grad(rank, it, n=N):
    g = torch.Generator().manual_seed(1000 * rank + it)
    return torch.randn(n, generator=g)


def _engine(comp, flag, warmup=2):
    import torch.distributed as dist

    from oktopk_amd import AllReducer, Comm, EngineConfig
    from oktopk_amd.config import OkTopkConfig

    kw = {"gaussian_device_select": True} if flag else {}
    cfg = EngineConfig(compressor=comp, density=DENSITY,
                       oktopk=OkTopkConfig(dense_warmup_iters=warmup), **kw)
    return AllReducer(Comm(dist.group.WORLD), cfg)


def _engine_invariants(rank):
    import torch.distributed as dist

    world = dist.get_world_size()
    for comp in COMPS:
        eng = _engine(comp, True)
        out_sum = torch.zeros(N)
        in_sum = torch.zeros(N)
        for it in range(ITERS):
            t = _grad(rank, it)
            in_sum += t
            out = eng.run("w", t.clone())
            out_sum += out
            # identical on every rank
            ref = out.clone()
            dist.broadcast(ref, src=0)
            assert torch.equal(out, ref), (comp, it)
        # mass conservation (tests/test_allreducer_dist.py): the sum over
        # ranks of (sent + residual) equals the restored input
        dist.all_reduce(in_sum)
        res = eng.states["w"].residual.clone()
        dist.all_reduce(res)
        err = (world * out_sum + res - in_sum).abs().max().item()
        assert err < 1e-3, f"{comp}: EF mass leak {err}"
        # the sparse iterations really selected something
        assert 0 < int((out != 0).sum()) < N // 2, comp


def _engine_bf16_grad_src(rank):
    for comp in COMPS:
        a, b = _engine(comp, True, warmup=1), _engine(comp, True, warmup=1)
        for it in range(4):
            g16 = _grad(rank, it).bfloat16()
            oa = a.run("w", torch.full((N,), 123.0), grad_src=g16)
            ob = b.run("w", g16.float())
            assert torch.equal(oa, ob), (comp, it)
        assert torch.equal(a.states["w"].residual, b.states["w"].residual)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_engine_device_select(world):
    run_dist(_engine_invariants, world)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_engine_device_select_bf16_grad_src(world):
    run_dist(_engine_bf16_grad_src, world)


def _flag_off_outputs(rank):
    outs = {}
    for comp in COMPS:
        eng = _engine(comp, False, warmup=1)
        acc = []
        for it in range(4):
            acc.append(eng.run("w", _grad(rank, it, 4096)).clone())
        outs[comp] = torch.stack(acc[1:])
    return outs


def _flag_off_matches_golden(rank):
    want = torch.load(GOLDEN)
    got = _flag_off_outputs(rank)
    for comp in COMPS:
        assert torch.equal(got[comp], want[comp]), comp


def test_flag_off_is_unchanged_world2():
    """With the flag off (the default) run() reproduces, bit for bit, the
    outputs recorded from the code before the device path existed."""
    run_dist(_flag_off_matches_golden, 2)
