"""CPU side of the core-kernel tests: the bit-rule selection helper, the
fp64 Adam oracle and its bounds (the torch composition passes them, each
mutant of it breaks one), the bit-level emulation of adam_f2b, and the
closed-form expectations test_core_kernels_gpu.py relies on."""
import math

import pytest
import torch

import core_cases as C
from oktopk_amd.ops import reference as R


# -- the bit rule -------------------------------------------------------------

def test_sel_gt_on_special_values():
    t = C.from_bits(torch.tensor(C.SPECIAL_BITS, dtype=torch.int64))
    nan, inf = torch.isnan(t), torch.isinf(t)
    assert int(nan.sum()) == 4 and int(inf.sum()) == 2
    for tau in (0.0, 0.1, 1.0, C.FLT_MAX):
        sel = R._sel_gt(t, tau)
        assert bool(sel[nan].all()) and bool(sel[inf].all())
    sel = R._sel_gt(t, C.INF)            # only NaN is above +inf
    assert torch.equal(sel, nan)
    for payload in C.NAN_PAYLOADS:       # a NaN tau is compared by its bits
        tau = float(C.from_bits(torch.tensor([payload])))
        tb = int(C.bits(torch.tensor([tau], dtype=torch.float32))) & 0x7FFFFFFF
        assert torch.equal(R._sel_gt(t, tau),
                           (C.bits(t) & 0x7FFFFFFF) > tb)
    # +-0 are never above tau = 0 (and -0.0 as a tau is 0), subnormals are
    zero = t == 0
    for tau in (0.0, -0.0):
        sel = R._sel_gt(t, tau)
        assert not bool(sel[zero].any()) and bool(sel[~zero].all())
    # tau < 0 selects everything, +-0 included; a double that rounds to
    # -0.0f is not below zero
    assert bool(R._sel_gt(t, -1e-30).all())
    assert torch.equal(R._sel_gt(t, -1e-60), R._sel_gt(t, 0.0))
    # strict: an element's own magnitude excludes it, one bit below takes it
    x = torch.tensor([0.75, -0.75, 0.5])
    assert R._sel_gt(x, 0.75).tolist() == [False, False, False]
    assert R._sel_gt(x, C.prev_toward_zero(0.75)).tolist() == [True, True, False]
    # tau is rounded to fp32 first: 0.1 -> 0x3dcccccd, above the double 0.1
    f01 = float(torch.tensor(0.1, dtype=torch.float32))
    y = torch.tensor([f01, C.prev_toward_zero(f01)])
    assert R._sel_gt(y, 0.1).tolist() == [False, False]


@pytest.mark.parametrize("kind", [k for k in C.KINDS if k != "special"])
@pytest.mark.parametrize("n", [1, 9, 513, 6145, 65537])
def test_sel_gt_is_abs_gt_without_nan(kind, n):
    t = C.make(kind, n)
    for tau in C.thresholds(kind, n):
        old = t.abs() > tau if tau >= 0 else torch.ones(n, dtype=torch.bool)
        assert torch.equal(R._sel_gt(t, tau), old)
        assert R.count_gt(t, tau) == int(old.sum())
        idx, val = R.compact_gt(t, tau)
        assert torch.equal(idx.long(), old.nonzero().reshape(-1))
        assert torch.equal(C.bits(val), C.bits(t[old]))


def test_nan_is_selected_everywhere_on_the_cpu_path():
    t = C.make("special", 513)
    nan = torch.isnan(t)
    for tau in (0.0, 1.0, C.INF):
        idx, val = R.compact_gt(t, tau)
        assert set(nan.nonzero().reshape(-1).tolist()) <= set(idx.tolist())
        assert R.count_multi_gt(t, [tau, -1.0]) == [idx.numel(), 513]
    res = t.clone()
    out = torch.zeros(513)
    i = torch.arange(513, dtype=torch.int32)
    cnt = R.scatter_gt_credit_(out, res, i, t, C.FLT_MAX)
    assert cnt == int((nan | torch.isinf(t)).sum())
    assert not bool(torch.isnan(res).any())   # the credit took the NaNs
    res2 = t.clone()
    assert R.credit_gt_(res2, i, t, C.FLT_MAX) == cnt
    assert torch.equal(C.bits(res2), C.bits(res))
    assert torch.equal(R._sparse_kept(t, C.FLT_MAX), nan | torch.isinf(t))


# -- closed forms the GPU tests use -----------------------------------------------

@pytest.mark.parametrize("n", C.SIZES_SMALL + C.SIZES_LARGE)
def test_edges_closed_form_equals_reference(n):
    t = C.make("edges", n)
    idx, val = R.compact_gt(t, 0.5)
    e_idx, e_val = C.edges_expected(n)
    assert torch.equal(idx, e_idx) and torch.equal(C.bits(val), C.bits(e_val))
    assert bool((e_idx[1:] > e_idx[:-1]).all())
    assert R.count_gt(t, 0.0) == e_idx.numel()


def test_sizes_hit_the_geometry_they_are_named_for():
    assert C.compact_geom(4_194_304) == (2048, 2048)  # one step per wave up to here
    assert C.compact_geom(4_194_299) == (2048, 2048)
    assert C.compact_geom(4_196_358) == (4096, 1025)
    assert C.compact_geom(8_390_011) == (6144, 1366)
    assert 8_390_011 - 1365 * 6144 < 6144 // 4 * 3    # last block: a wave idle
    assert sorted({n % 8 for n in C.EF_SIZES})[1:] == [1, 2, 3, 4, 5, 6, 7]
    sub = C.make("subnormal_only", 513)
    assert int((C.bits(sub) & 0x7FFFFFFF).max()) < 1 << 21
    low = C.bits(C.make("low_bits", 513)) & 0x7FFFFFFF
    assert len(set((low >> 10).tolist())) == 1 and len(set(low.tolist())) > 100
    mid = C.bits(C.make("mid_bits", 513)) & 0x7FFFFFFF
    assert len(set((mid >> 21).tolist())) == 1
    assert len(set((mid & 0x3FF).tolist())) == 1 and len(set(mid.tolist())) > 100
    assert not bool((C.make("dense", 65537) == 0).any())


@pytest.mark.parametrize("kind", ["randn", "quant", "special", "low_bits"])
def test_sorted_magnitudes_index_equals_kth_abs_value(kind):
    # the large GPU cases index one descending sort instead of one topk per k
    n = 6145
    t = C.make(kind, n)
    vals = torch.topk(t.abs(), n, sorted=True).values
    for k in (1, 2, 6, n // 2, n - 1, n):
        a, b = R.kth_abs_value(t, k), float(vals[k - 1])
        assert a == b or (math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("n", C.NORM_SIZES)
def test_integer_sum_of_squares_is_exact_in_fp64_any_order(n):
    t, exact = C.norm_case("integer", n)
    sq = t.double() ** 2
    assert float(sq.sum()) == exact == float(sq.flip(0).sum())
    assert float(torch.cumsum(sq, 0)[-1]) == exact
    assert exact < 2 ** 53


# -- adam_f2b ------------------------------------------------------------------

def test_f2b_emulation_equals_torch_cast():
    crafted = C.from_bits(torch.tensor(
        C.MIRROR_FINITE_BITS + C.MIRROR_NONFINITE_BITS, dtype=torch.int64))
    g = torch.Generator().manual_seed(5)
    rnd = C.from_bits(torch.randint(-(1 << 31), 1 << 31, (1_000_000,),
                                    generator=g))
    for x in (crafted, rnd):
        mine, ref = C.f2b_emulated(x), x.to(torch.bfloat16)
        nan = torch.isnan(x)
        assert torch.equal(torch.isnan(mine), nan)
        assert torch.equal(torch.isnan(ref), nan)
        assert torch.equal(mine.view(torch.int16)[~nan],
                           ref.view(torch.int16)[~nan])
        # the select changes nothing but NaN
        old = C.f2b_parent(x)
        assert torch.equal(old.view(torch.int16)[~nan],
                           mine.view(torch.int16)[~nan])
    # sign and upper payload survive, the quiet bit is set
    out = C.f2b_emulated(C.from_bits(torch.tensor(C.NAN_PAYLOADS)))
    assert [v & 0xFFFF for v in out.view(torch.int16).tolist()] == [
        0x7FC0, 0xFFC0, 0x7FC0, 0x7FFF]


def test_f2b_without_the_select_corrupts_nan():
    x = C.from_bits(torch.tensor(
        [0x7FFFFFFF, 0x7FFF8000, 0xFFFFFFFF - (1 << 32), 0x7F800001]))
    old = C.f2b_parent(x).view(torch.int16).tolist()
    assert [v & 0xFFFF for v in old] == [0x8000, 0x8000, 0x0000, 0x7F80]


# -- adam_ref64 / adam_bounds -----------------------------------------------------

def _ratios(p0, g, m0, v0, p1, m1, v1, hp, wd, gs):
    """max |x' - x64| / bound per tensor, p judged from the given m', v'."""
    args = (hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, gs)
    m64, v64, p_of = R.adam_ref64(p0, g, m0, v0, *args)
    bm, bv, bp = R.adam_bounds(p0, g, m0, v0, m1, v1, *args)
    return (float(((m1.double() - m64).abs() / bm).max()),
            float(((v1.double() - v64).abs() / bv).max()),
            float(((p1.double() - p_of(m1, v1)).abs() / bp).max()))


def _torch_adam(p, g, m, v, hp, wd, gs, mutant=None):
    """R.fused_adam_'s composition on clones; `mutant` alters one thing."""
    p, m, v = p.clone(), m.clone(), v.clone()
    lr, b1, b2, eps = hp["lr"], hp["b1"], hp["b2"], hp["eps"]
    if mutant is None:
        R.fused_adam_(p, g, m, v, lr, b1, b2, eps, wd,
                      None if gs is None else torch.tensor([gs]))
        return p, m, v
    gi = g if gs is None else g * gs
    if mutant == "betas_swapped":
        b1, b2 = b2, b1
    c2 = 0.001 if mutant == "c2_double" else 1 - b2
    m.mul_(b1).add_(gi, alpha=1 - b1)
    g2 = g if mutant == "unscaled_g" else gi
    v.mul_(b2).addcmul_(gi, g2, value=c2)
    if mutant == "eps_inside":
        update = m / (v + eps * eps).sqrt()
    else:
        update = m / (v.sqrt() + eps)
    if mutant == "bias_corrected":
        update = update * (math.sqrt(1 - b2) / (1 - b1))
    if mutant == "wd_after":
        p.add_(update, alpha=-lr)
        p.mul_(1 - lr * wd)
    else:
        p.add_(update + wd * p, alpha=-lr)
    return p, m, v


@pytest.mark.parametrize("gs", C.ADAM_GSCALES)
@pytest.mark.parametrize("wd", C.ADAM_WD["exact"])
@pytest.mark.parametrize("n", [5, 1025, 100_003])
def test_torch_composition_is_within_the_bounds(n, wd, gs):
    """On the binary-exact hyperparameters torch's own convention (doubles,
    1 - b as a double) and the kernel's coincide, so R.fused_adam_ must sit
    inside the bounds, on every stretch of the data."""
    hp = C.ADAM_HYPER["exact"]
    p, g, m, v = C.adam_case(n, "exact")
    for _ in range(3):
        p1, m1, v1 = _torch_adam(p, g, m, v, hp, wd, gs)
        rm, rv, rp = _ratios(p, g, m, v, p1, m1, v1, hp, wd, gs)
        assert rm <= 1 and rv <= 1 and rp <= 1, (rm, rv, rp)
        p, m, v = p1, m1, v1
    s = torch.arange(n) % C.ADAM_STRETCHES  # per stretch, for the record
    for k in range(min(n, C.ADAM_STRETCHES)):
        sel = s == k
        r = _ratios(p[sel], g[sel], m[sel], v[sel],
                    *[x[sel] for x in _torch_adam(p, g, m, v, hp, wd, gs)],
                    hp, wd, gs)
        assert max(r) <= 1, (k, r)


# mutant -> (hyperparameter set, wd, gscale, index of the tensor it breaks)
MUTANTS = {
    "eps_inside": ("exact", 0.0, None, 2),
    "wd_after": ("exact", 2.0 ** -7, None, 2),
    "unscaled_g": ("exact", 0.0, 0.375, 1),
    "betas_swapped": ("exact", 0.0, None, 0),
    "bias_corrected": ("exact", 0.0, None, 2),
    "c2_double": ("production", 0.0, None, 1),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_each_mutant_breaks_a_bound(mutant):
    hyper, wd, gs, which = MUTANTS[mutant]
    hp = C.ADAM_HYPER[hyper]
    p, g, m, v = C.adam_case(100_003, hyper)
    r = _ratios(p, g, m, v, *_torch_adam(p, g, m, v, hp, wd, gs, mutant),
                hp, wd, gs)
    print(mutant, "ratios m, v, p:", r)
    assert r[which] > 4, r


def test_wd_after_mutant_breaks_p_on_the_production_set_too():
    hp = C.ADAM_HYPER["production"]
    p, g, m, v = C.adam_case(100_003, "production")
    r = _ratios(p, g, m, v, *_torch_adam(p, g, m, v, hp, 0.01, None, "wd_after"),
                hp, 0.01, None)
    assert r[2] > 4, r


def test_double_convention_misses_the_v_bound_at_production_values():
    """Why the oracle is not R.fused_adam_: its 1 - b2 is the double 0.001,
    the kernel's is fp32(1 - fp32(0.999))."""
    hp = C.ADAM_HYPER["production"]
    p, g, m, v = C.adam_case(100_003, "production")
    r = _ratios(p, g, m, v, *_torch_adam(p, g, m, v, hp, 0.0, None), hp, 0.0,
                None)
    print("R.fused_adam_ at production values, ratios m, v, p:", r)
    assert r[1] > 4


def test_adam_hyper_convention():
    lr, b1, b2, eps, wd, gs, c1, c2 = R.adam_hyper_f32(2e-4, 0.9, 0.999, 1e-6,
                                                      0.01)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    assert (lr, b1, b2, eps, wd, gs) == (f32(2e-4), f32(0.9), f32(0.999),
                                         f32(1e-6), f32(0.01), 1.0)
    one = torch.tensor(1.0)
    assert c1 == float(one - torch.tensor(0.9)) != 1 - 0.9
    assert c2 == float(one - torch.tensor(0.999)) != 1 - 0.999
    assert R.adam_hyper_f32(1, 0.875, 0.5, 1, 0, torch.tensor([0.375]))[5:] == (
        0.375, 0.125, 0.5)
