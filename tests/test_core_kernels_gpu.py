"""The round-1/2 kernels of ops/csrc/kernels.hip — selection, error
feedback, radix select, dense Adam, norms, scatters — against the torch
reference, at the sizes where the compact geometry changes path and on
planted bit patterns (cases: core_cases.py).

Everything but Adam and the norms copies a float, adds two floats once or
counts, so it is compared bit for bit (int32 views: -0 and NaN payloads
count).  Adam is judged element by element against the fp64 oracle
R.adam_ref64 within R.adam_bounds; the sums of squares against the exact
sum."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import core_cases as C
from core_cases import bits, shifted
from oktopk_amd import ops
from oktopk_amd.ops import reference as R


def hip():
    from oktopk_amd import _hip_ops

    return _hip_ops


def _same(a, b):
    """Bit equality of a GPU/CPU fp32 (or bf16) result with a CPU one."""
    a, b = a.cpu(), b.cpu()
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _cached(store, group, key, make):
    """CPU references are computed once per case and shared by the tests
    that need them; a store keeps one (kind, n) group at a time, so the
    references of the multi-million-element cases do not pile up."""
    if store.get("group") != group:
        store.clear()
        store["group"] = group
    if key not in store:
        store[key] = make()
    return store[key]


# -- a. compact_gt, count_gt, count_multi_gt, compact_adaptive ----------------------

_compact_refs = {}


def _ref_compact(kind, n, tau):
    return _cached(_compact_refs, (kind, n), tau,
                   lambda: R.compact_gt(C.make(kind, n), tau))


@pytest.mark.parametrize("place", ["aligned", "shifted"])
@pytest.mark.parametrize("kind,n", C.kind_size_params())
def test_compact_and_counts_match_bit_rule(kind, n, place):
    t = C.make(kind, n)
    dt = shifted(t) if place == "shifted" else t.cuda()
    taus = C.thresholds(kind, n)
    want_counts = []
    for tau in taus:
        o_idx, o_val = _ref_compact(kind, n, tau)
        idx, val = ops.compact_gt(dt, tau)
        assert idx.dtype == torch.int32 and val.dtype == torch.float32
        assert torch.equal(idx.cpu(), o_idx), tau
        assert _same(val, o_val), tau
        if idx.numel() > 1:
            assert bool((idx[1:] > idx[:-1]).all())
        assert ops.count_gt(dt, tau) == o_idx.numel(), tau
        want_counts.append(o_idx.numel())
    assert want_counts[0] == n                      # tau < 0: everything
    assert want_counts[-1] == int(torch.isnan(t).sum())  # +inf: NaN only
    assert ops.count_multi_gt(dt, taus) == want_counts
    assert ops.count_multi_gt(dt, taus[:1]) == want_counts[:1]
    assert _same(dt, t)                             # nothing is written


@pytest.mark.parametrize("place", ["aligned", "shifted"])
@pytest.mark.parametrize("n", C.sizes_for("edges"))
def test_edges_compaction_closed_form(n, place):
    """No reference involved: the planted positions, in order."""
    t = C.make("edges", n)
    dt = shifted(t) if place == "shifted" else t.cuda()
    e_idx, e_val = C.edges_expected(n)
    for tau in (0.5, 0.0):
        idx, val = ops.compact_gt(dt, tau)
        assert torch.equal(idx.cpu(), e_idx) and _same(val, e_val)
        assert ops.count_gt(dt, tau) == e_idx.numel()
    idx, val, chosen, cnt = ops.compact_adaptive(dt, [0.0, 0.5, 1.0], 0)
    assert (chosen, cnt, idx.numel()) == (2, 0, 0)  # 1.0 is excluded: strict


@pytest.mark.parametrize("place", ["aligned", "shifted"])
@pytest.mark.parametrize("n", C.sizes_for("dense"))
def test_dense_selects_every_element(n, place):
    """tau < 0 and tau = 0 on data without a zero: every lane stores all 8
    of its elements in every step; the output is the input."""
    t = C.make("dense", n)
    dt = shifted(t) if place == "shifted" else t.cuda()
    for tau in (-1.0, 0.0):
        idx, val = ops.compact_gt(dt, tau)
        assert torch.equal(idx.cpu(), torch.arange(n, dtype=torch.int32))
        assert _same(val, t)


@pytest.mark.parametrize("place", ["aligned", "shifted"])
@pytest.mark.parametrize("kind,n", C.kind_size_params())
def test_compact_adaptive_matches_reference(kind, n, place):
    t = C.make(kind, n)
    dt = shifted(t) if place == "shifted" else t.cuda()
    for taus, hi_limit, expect in C.adaptive_cases(kind, n):
        o_idx, o_val, o_chosen, o_cnt = R.compact_adaptive(t, taus, hi_limit)
        if expect is not None:
            assert o_chosen == expect
        idx, val, chosen, cnt = ops.compact_adaptive(dt, taus, hi_limit)
        assert (chosen, cnt) == (o_chosen, o_cnt), (taus, hi_limit)
        assert torch.equal(idx.cpu(), o_idx) and _same(val, o_val)
    assert _same(dt, t)


# -- b. compact_adaptive_ef -------------------------------------------------------------

_ef_refs = {}


def _ref_ef(kind, n, j):
    """R.compact_adaptive_ef for tau set j: (idx, val, chosen, cnt, residual)."""
    def make():
        t, r, grad = C.ef_case(kind, n)
        taus, hi = C.ef_tau_sets(kind, n)[j]
        o_r = r.clone()
        out = R.compact_adaptive_ef(t.clone(), o_r, grad, taus, hi)
        return (*out, o_r)

    return _cached(_ef_refs, (kind, n), j, make)


def _ef_shift_params(shifts):
    """(kind, n, shift) below the multi-million sizes; `grad` only where the
    kind has a bf16 gradient."""
    return [(k, n, s) for k, n in C.ef_params() if n <= 1_000_003
            for s in shifts if s != "grad" or C.ef_case(k, 1)[2] is not None]


def _ef_device(kind, n, shift=None):
    t, r, grad = C.ef_case(kind, n)
    put = lambda x, name: shifted(x) if shift == name else x.cuda()
    return (put(t, "t"), put(r, "residual"),
            None if grad is None else put(grad, "grad"))


@pytest.mark.parametrize("via", ["ops", "binding"])
@pytest.mark.parametrize("kind,n", C.ef_params())
def test_compact_adaptive_ef_matches_reference(kind, n, via):
    t, r, grad = C.ef_case(kind, n)
    if kind == "infnan" and n >= 10:
        assert bool(torch.isnan(C.ef_restored(kind, n)).any())
    fn = ops.compact_adaptive_ef if via == "ops" else hip().compact_adaptive_ef
    for j, (taus, hi) in enumerate(C.ef_tau_sets(kind, n)):
        o_idx, o_val, o_chosen, o_cnt, o_r = _ref_ef(kind, n, j)
        dt, dr, dg = _ef_device(kind, n)
        idx, val, chosen, cnt = fn(dt, dr, dg, taus, hi)
        assert (int(chosen), int(cnt)) == (o_chosen, o_cnt)
        assert torch.equal(idx.cpu(), o_idx) and _same(val, o_val)
        assert _same(dr, o_r)
        assert _same(dt, t)  # t is not written
        if dg is not None:
            assert _same(dg, grad)
    # NaN sums are selected at every tau, +0 sums at none but tau < 0
    restored = C.ef_restored(kind, n)
    o_idx = _ref_ef(kind, n, 1)[0]
    assert o_idx.numel() == int((restored != 0).sum())


@pytest.mark.parametrize("kind,n,shift",
                         _ef_shift_params(["t", "residual", "grad"]))
def test_compact_adaptive_ef_unaligned(kind, n, shift):
    """ops.compact_adaptive_ef on a buffer that is only 4-byte aligned takes
    the unfused route (scalar restore + compact_adaptive); the binding
    refuses such a buffer."""
    t, r, grad = C.ef_case(kind, n)
    restored = C.ef_restored(kind, n)
    for j, (taus, hi) in enumerate(C.ef_tau_sets(kind, n)):
        o_idx, o_val, o_chosen, o_cnt, o_r = _ref_ef(kind, n, j)
        dt, dr, dg = _ef_device(kind, n, shift)
        idx, val, chosen, cnt = ops.compact_adaptive_ef(dt, dr, dg, taus, hi)
        assert (chosen, cnt) == (o_chosen, o_cnt)
        assert torch.equal(idx.cpu(), o_idx) and _same(val, o_val)
        assert _same(dr, o_r)
        # t holds its input or the restored values, nothing else
        assert _same(dt, t) or _same(dt, restored)
    dt, dr, dg = _ef_device(kind, n, shift)
    with pytest.raises(RuntimeError):
        hip().compact_adaptive_ef(dt, dr, dg, [0.5], n)
    assert _same(dr, r) and _same(dt, t)  # refused before any write


# -- c. ef_restore_snapshot_, ef_restore_upcast_ ----------------------------------------

@pytest.mark.parametrize("kind,n,shift",
                         _ef_shift_params([None, "t", "residual", "grad"]))
def test_ef_restore_matches_reference(kind, n, shift):
    t, r, grad = C.ef_case(kind, n)
    o_t, o_r = t.clone(), r.clone()
    dt, dr, dg = _ef_device(kind, n, shift)
    if grad is None:
        R.ef_restore_snapshot_(o_t, o_r)
        out = ops.ef_restore_snapshot_(dt, dr)
    else:
        R.ef_restore_upcast_(o_t, o_r, grad)
        out = ops.ef_restore_upcast_(dt, dr, dg)
        assert _same(dg, grad)
    assert out.data_ptr() == dt.data_ptr()
    assert _same(dt, o_t) and _same(dr, o_r)
    assert _same(dt, dr)


# -- d. kth_abs_value ---------------------------------------------------------------------

_sorted_abs = {}


def _ref_kth(kind, n, k):
    """R.kth_abs_value(t, k); at the three largest sizes read from one
    descending torch.topk(|t|, n) — R.kth_abs_value's own computation at
    k = n, whose entry k-1 is its answer for k (checked on the CPU in
    test_core_kernels_reference.py) — instead of one topk per k."""
    t = C.make(kind, n)
    if n <= 1_000_003:
        return R.kth_abs_value(t, k)
    vals = _cached(_sorted_abs, (kind, n), "sorted",
                   lambda: torch.topk(t.abs(), n, sorted=True).values)
    return float(vals[max(1, min(int(k), n)) - 1])


def _eq_or_both_nan(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _quiet_or_no_nan(abs_bits):
    return abs_bits <= 0x7F800000 or bool(abs_bits & 0x00400000)


@pytest.mark.parametrize("kind,n", C.kind_size_params())
def test_kth_abs_value_exact_and_brackets(kind, n):
    t = C.make(kind, n)
    dt = t.cuda()
    for k in sorted({0, 1, 2, n // 1000, n // 2, n - 1, n, n + 5}):
        want = _ref_kth(kind, n, k)
        tau = ops.kth_abs_value(dt, k)
        assert _eq_or_both_nan(tau, want), (k, tau, want)
        assert _eq_or_both_nan(ops.topk_select(dt, max(1, k))[2], tau), k
        kk = max(1, min(k, n))
        # the bracket: fewer than k above tau, at least k above the next
        # pattern towards zero (tau < 0, everything, when tau is 0)
        if math.isnan(tau):
            # A threshold crosses the Python API as a double, and the
            # float <-> double conversions set a NaN's quiet bit: a
            # signalling pattern cannot be passed in or out.  Each side of
            # the bracket is asserted where its pattern survives the trip
            # (0x7fffffff and 0x7ffffffe do; 0x7fc00000 - 1 does not).
            kth_bits = int((bits(t) & 0x7FFFFFFF).sort().values[n - kk])
            if _quiet_or_no_nan(kth_bits):
                assert ops.count_gt(dt, tau) < kk
                if _quiet_or_no_nan(kth_bits - 1):
                    below = float(C.from_bits(torch.tensor([kth_bits - 1])))
                    assert ops.count_gt(dt, below) >= kk
            continue
        assert ops.count_gt(dt, tau) < kk
        below = C.prev_toward_zero(tau) if tau != 0 else -1.0
        assert ops.count_gt(dt, below) >= kk
    assert _same(dt, t)


# -- e. fused_adam_, fused_adam_mirror_ ---------------------------------------------------

ADAM_PATHS = ["float4", "shift_p", "shift_g", "shift_m", "shift_v",
              "shift_mirror"]
# (tensor, float4 | scalar, hyperparameter set) -> largest error / bound seen
adam_worst = {}


def _adam_runs(path, wd):
    """Which op(s) a combination runs: both on the float4 path, the mirror
    op where the mirror is shifted, and one of each on the other shifts."""
    if path == "float4":
        return [False, True]
    if path == "shift_mirror":
        return [True]
    return [wd != 0]


def _adam_step_checked(n, path, hyper, wd, gs, mirror):
    hp = C.ADAM_HYPER[hyper]
    args = (hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd)
    p, g, m, v = C.adam_case(n, hyper)
    put = lambda x, name: shifted(x) if path == "shift_" + name else x.cuda()
    dp, dg, dm, dv = put(p, "p"), put(g, "g"), put(m, "m"), put(v, "v")
    dgs = None if gs is None else torch.tensor([gs], device="cuda")
    db = None
    if mirror:
        db = put(torch.zeros(n, dtype=torch.bfloat16), "mirror")
    scalar = path != "float4"
    for step in range(3):  # each step judged from the kernel's own state
        p0, m0, v0 = dp.cpu(), dm.cpu(), dv.cpu()
        if mirror:
            ops.fused_adam_mirror_(dp, dg, dm, dv, db, *args, dgs)
        else:
            ops.fused_adam_(dp, dg, dm, dv, *args, dgs)
        p1, m1, v1 = dp.cpu(), dm.cpu(), dv.cpu()
        m64, v64, p_of = R.adam_ref64(p0, g, m0, v0, *args, gs)
        bm, bv, bp = R.adam_bounds(p0, g, m0, v0, m1, v1, *args, gs)
        errs = {"m": (m1.double() - m64).abs() / bm,
                "v": (v1.double() - v64).abs() / bv,
                "p": (p1.double() - p_of(m1, v1)).abs() / bp}
        for name, e in errs.items():
            worst = float(e.max())
            # float4 covers n - n % 4 elements, the scalar tail the rest
            kinds = (["scalar"] if scalar or n < 4 else
                     ["float4"] + (["scalar"] if n % 4 else []))
            for kd in kinds:
                sl = (slice(None) if scalar or n < 4 else
                      slice(0, n - n % 4) if kd == "float4" else
                      slice(n - n % 4, n))
                key = (name, kd, hyper)
                adam_worst[key] = max(adam_worst.get(key, 0.0),
                                      float(e[sl].max()))
            assert worst <= 1.0, (name, step, wd, gs, mirror, worst,
                                  int(e.argmax()))
        assert _same(dg, g)
        if mirror:
            assert _same(db, p1.to(torch.bfloat16))
    return dp, dm, dv, db


@pytest.mark.parametrize("hyper", sorted(C.ADAM_HYPER))
@pytest.mark.parametrize("path", ADAM_PATHS)
@pytest.mark.parametrize("n", C.ADAM_SIZES)
def test_adam_within_bounds_of_fp64(n, path, hyper):
    for wd in C.ADAM_WD[hyper]:
        for gs in C.ADAM_GSCALES:
            for mirror in _adam_runs(path, wd):
                _adam_step_checked(n, path, hyper, wd, gs, mirror)


def test_adam_ratio_record():
    """Prints the largest error-to-bound ratios the cases above produced
    (profiles/README.md r13); asserts only what they already asserted."""
    for key in sorted(adam_worst):
        print("adam error/bound", *key, "%.3f" % adam_worst[key])
        assert adam_worst[key] <= 1.0


@pytest.mark.parametrize("path", ["float4", "shift_p"])
@pytest.mark.parametrize("n", [5, 1025, 100_003])
def test_adam_gscale_one_is_no_gscale(n, path):
    hyper = "production"
    a = _adam_step_checked(n, path, hyper, 0.01, None, True)
    b = _adam_step_checked(n, path, hyper, 0.01, 1.0, True)
    for x, y in zip(a, b):
        assert _same(x, y)


@pytest.mark.parametrize("path", ["float4", "shift_mirror", "shift_p"])
def test_adam_mirror_of_crafted_weights(path):
    """lr = 0, wd = 0 and zero moments and gradient: the update is p - 0*0,
    so a finite p keeps its bits and the mirror is its bf16 rounding — ties
    to even on both parities, the carry into the next exponent, FLT_MAX to
    inf, subnormals, -0.  For p = +-inf the formula itself gives NaN
    (wd*p = 0*inf), as the fp64 oracle does; for NaN p the result is NaN.
    Wherever p' is NaN the mirror must be NaN: the rounding carry alone
    would make -0.0, +0.0 or inf of some payloads."""
    fin = C.from_bits(torch.tensor(C.MIRROR_FINITE_BITS, dtype=torch.int64))
    non = C.from_bits(torch.tensor(C.MIRROR_NONFINITE_BITS, dtype=torch.int64))
    # three copies and n % 4 == 3: crafted values in the float4 loop and in
    # the scalar tail
    body = torch.cat([fin, non] * 3)
    pad = (3 - (body.numel() + 2)) % 4
    p = torch.cat([body, fin[:pad], non[-2:]])
    n = p.numel()
    assert n % 4 == 3
    finite = torch.isfinite(p)
    z = torch.zeros(n)
    put = lambda x, name: shifted(x) if path == "shift_" + name else x.cuda()
    dp, db = put(p, "p"), put(torch.ones(n, dtype=torch.bfloat16), "mirror")
    dg, dm, dv = z.cuda(), z.cuda(), z.cuda()
    ops.fused_adam_mirror_(dp, dg, dm, dv, db, 0.0, 0.9, 0.999, 1e-6, 0.0)
    p1, b1 = dp.cpu(), db.cpu()
    print("p' bits of the non-finite inputs:",
          [hex(x & 0xFFFFFFFF) for x in bits(p1)[~finite].tolist()],
          "mirror:", [hex(x & 0xFFFF) for x in
                      b1.view(torch.int16)[~finite].tolist()])
    assert torch.equal(bits(p1)[finite], bits(p)[finite])
    assert bool(torch.isnan(p1[~finite]).all())
    _, _, p_of = R.adam_ref64(p, z, z, z, 0.0, 0.9, 0.999, 1e-6, 0.0)
    assert torch.equal(torch.isnan(p_of(z, z)), ~finite)
    assert torch.equal(b1.view(torch.int16)[finite],
                       p.to(torch.bfloat16).view(torch.int16)[finite])
    assert _same(b1[finite], C.f2b_emulated(p)[finite])
    assert bool(torch.isnan(b1[~finite]).all())
    assert not bool(dm.any()) and not bool(dv.any())


# -- f. l2norm, sumsq_into_, grad_clip_scale, clip_scale_from_sumsq ------------------------

def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _ulp32(x):
    a = torch.tensor(abs(x), dtype=torch.float32)
    return float(torch.nextafter(a, torch.tensor(C.INF)) - a)


@pytest.mark.parametrize("place", ["aligned", "shifted"])
@pytest.mark.parametrize("n", C.NORM_SIZES)
@pytest.mark.parametrize("kind", ["integer", "randn"])
def test_sum_of_squares_against_exact(kind, n, place):
    t, exact = C.norm_case(kind, n)
    dt = shifted(t) if place == "shifted" else t.cuda()
    # integer: exact in fp64 in any order.  randn: non-negative terms, each
    # exact in fp64, so any summation order is within n*2^-53 relative
    tol = 0.0 if kind == "integer" else n * 2.0 ** -53 * exact
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    ops.sumsq_into_(acc, dt)
    got = float(acc)
    assert abs(got - exact) <= tol, (got, exact)
    ops.sumsq_into_(acc, dt)            # accumulates, here a second tensor
    t2, exact2 = C.norm_case(kind, C.NORM_SIZES[(C.NORM_SIZES.index(n) + 3)
                                                % len(C.NORM_SIZES)])
    ops.sumsq_into_(acc, t2.cuda())
    total = 2 * exact + exact2
    tol3 = (0.0 if kind == "integer"
            else (2 * n + t2.numel() + 3) * 2.0 ** -53 * total)
    assert abs(float(acc) - total) <= tol3
    # l2norm: the host's correctly rounded sqrt of the same sum
    norm = ops.l2norm(dt)
    if kind == "integer":
        assert norm == math.sqrt(exact)
    else:
        assert abs(norm - math.sqrt(exact)) <= (n + 2) * 2.0 ** -53 * math.sqrt(exact)
    # the clip factor: 1 when the norm fits, else fp32(max / (norm + 1e-6))
    gn = math.sqrt(exact)
    for mx in (gn * 2 + 1, gn * 0.37 + 1e-3):
        want = 1.0 if gn <= _f32(mx) else _f32(_f32(mx) / (gn + 1e-6))
        for got in (float(ops.grad_clip_scale(dt, mx)),
                    float(ops.clip_scale_from_sumsq(
                        torch.tensor([float(exact)], dtype=torch.float64,
                                     device="cuda"), mx))):
            if want == 1.0:
                assert got == 1.0
            else:
                assert abs(got - want) <= _ulp32(want), (got, want)
    assert _same(dt, t)


@pytest.mark.parametrize("place", ["aligned", "shifted"])
def test_clip_factor_at_the_threshold(place):
    t = torch.tensor([3.0, 4.0])
    dt = shifted(t) if place == "shifted" else t.cuda()
    assert ops.l2norm(dt) == 5.0
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    ops.sumsq_into_(acc, dt)
    assert float(acc) == 25.0
    # the norm equal to max_norm does not clip: exactly 1.0f
    for s in (ops.grad_clip_scale(dt, 5.0), ops.clip_scale_from_sumsq(acc, 5.0),
              ops.grad_clip_scale(dt, 6.0)):
        assert s.dtype == torch.float32 and s.numel() == 1
        assert float(s) == 1.0
    # one fp32 pattern below 5 must fire
    below = C.prev_toward_zero(5.0)
    want = _f32(below / (5.0 + 1e-6))
    for s in (ops.grad_clip_scale(dt, below),
              ops.clip_scale_from_sumsq(acc, below)):
        assert float(s) < 1.0
        assert abs(float(s) - want) <= _ulp32(want)
    # and it matches the reference's own composition to the bit
    assert _same(ops.clip_scale_from_sumsq(acc, below),
                 R.clip_scale_from_sumsq(acc.cpu(), below))


# -- g. scatters ------------------------------------------------------------------------------

M_SIZES = [0, 1, 255, 256, 257, 600_001]


def _i32(x):
    return x.to(torch.int32)


@pytest.mark.parametrize("m", M_SIZES)
def test_scatter_add_with_heavy_duplicates(m):
    g = torch.Generator().manual_seed(m + 1)
    n = 1000
    # ~50 targets, integer values: every partial sum is exact, so the order
    # of the atomics cannot show
    idx = _i32(torch.randint(0, 50, (m,), generator=g) * 19 + 3)
    val = torch.randint(-8, 9, (m,), generator=g).float()
    dest = torch.randint(-4, 5, (n,), generator=g).float()
    want = R.scatter_add_(dest.clone(), idx, val)
    for put in (torch.Tensor.cuda, shifted) if m else (torch.Tensor.cuda,):
        d = put(dest)
        out = ops.scatter_add_(d, put(idx), put(val))
        assert out.data_ptr() == d.data_ptr()
        assert _same(d, want)


@pytest.mark.parametrize("m", M_SIZES)
def test_fill_zero_and_masked_zero_match_reference(m):
    g = torch.Generator().manual_seed(m + 2)
    n = max(2 * m, 64) + 3
    idx = _i32(torch.randperm(n, generator=g)[:m].sort().values)
    val = torch.randn(m, generator=g)
    val[::3] = 0.0    # +0 * negative scale = -0
    val[1::7] = -0.0
    base = torch.randn(n, generator=g)
    mask = torch.rand(n, generator=g) < 0.5
    for scale in (0.5, -0.25, 1.0):
        want = R.fill_sparse_scaled_(base.clone(), idx, val, scale)
        d = base.cuda()
        ops.fill_sparse_scaled_(d, idx.cuda(), val.cuda(), scale)
        assert _same(d, want)
        if m and scale < 0:  # val[0] is +0: the product is -0
            assert int(bits(want)[idx[0]]) == -(1 << 31)
    for put in (torch.Tensor.cuda, shifted) if m else (torch.Tensor.cuda,):
        want = R.zero_at_(base.clone(), idx)
        d = put(base)
        ops.zero_at_(d, put(idx))
        assert _same(d, want)
        want = R.zero_at_masked_(base.clone(), idx, mask)
        d = put(base)
        ops.zero_at_masked_(d, put(idx), mask.cuda())
        assert _same(d, want)


@pytest.mark.parametrize("m", M_SIZES)
def test_isin_sorted_matches_reference(m):
    g = torch.Generator().manual_seed(m + 3)
    lo, hi = -(1 << 31), (1 << 31) - 1
    b = torch.randint(-1000, 1000, (m,), generator=g).unique()  # ascending
    a = torch.randint(-1200, 1200, (max(m, 300),), generator=g)
    cases = [(a, b), (a[:0], b), (a, b[:0]), (a[:0], b[:0]),
             # below and above all of b, and the int32 limits on either side
             (torch.tensor([lo, -5000, 5000, hi, 0]), b),
             (torch.tensor([lo, hi, 0, 1, lo + 1, hi - 1]),
              torch.tensor([lo, 0, hi])),
             (torch.tensor([lo, hi]), torch.tensor([lo + 1, hi - 1]))]
    for x, y in cases:
        x, y = _i32(x), _i32(y)
        want = R.isin_sorted(x, y)
        got = ops.isin_sorted(x.cuda(), y.cuda())
        assert got.dtype == torch.bool
        assert torch.equal(got.cpu(), want), (x[:8], y[:8])


@pytest.mark.parametrize("m", M_SIZES)
def test_scatter_gt_credit_matches_reference(m):
    g = torch.Generator().manual_seed(m + 4)
    n = max(2 * m, 64) + 5
    idx = _i32(torch.randperm(n, generator=g)[:m].sort().values)
    val = torch.randn(m, generator=g)
    sp = C.from_bits(torch.tensor(C.SPECIAL_BITS, dtype=torch.int64))
    k = min(m, sp.numel())
    val[:k] = sp[:k]
    res0 = torch.randn(n, generator=g)
    out0 = torch.full((n,), 7.0)  # whatever is there stays where nothing lands
    taus = [-1.0, 0.0, 0.1, C.FLT_MAX, C.INF]
    e = C.an_element_magnitude(val) if m else None
    if e is not None:
        taus += [e, C.prev_toward_zero(e)]
    for tau in taus:
        for scale in (1.0, -0.5):
            o_out, o_res = out0.clone(), res0.clone()
            o_cnt = R.scatter_gt_credit_(o_out, o_res, idx, val, tau, scale)
            d_out, d_res = out0.cuda(), res0.cuda()
            cnt = ops.scatter_gt_credit_(d_out, d_res, idx.cuda(), val.cuda(),
                                         tau, scale)
            assert cnt == o_cnt, tau
            assert _same(d_out, o_out) and _same(d_res, o_res), tau
        o_res = res0.clone()
        o_cnt = R.credit_gt_(o_res, idx, val, tau)
        d_res = res0.cuda()
        assert ops.scatter_gt_credit_(None, d_res, idx.cuda(), val.cuda(),
                                      tau) == o_cnt
        assert _same(d_res, o_res)
        if tau < 0:
            assert o_cnt == m
