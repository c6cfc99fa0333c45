"""Ok-Topk round-1 reduce as an ordered sparse merge (ops.reduce_segments /
ops.reduce_segments_wire) on the CPU: the torch references against a dict
accumulated in segment order, named value cases, the wire form against the
pair form, argument checks, and the engine with OkTopkConfig.device_reduce
against the scatter-add composition over gloo.  Every comparison is bit for
bit; no tolerance appears anywhere."""
import numpy as np
import pytest
import torch

from conftest import run_dist
from oktopk_amd import ops
from oktopk_amd.config import EngineConfig, OkTopkConfig
from oktopk_amd.ops import reference as ref


def bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def brute(idx, val, counts, base, length, tau):
    """The op by other means: a dict of numpy fp32 scalars accumulated in
    segment order, entry by entry, starting from +0.0."""
    assert sum(counts) == idx.numel() == val.numel()
    acc = {}
    v32 = val.numpy()
    with np.errstate(all="ignore"):
        for x, v in zip(idx.tolist(), v32):
            if base <= x < base + length:
                acc[x] = np.float32(acc.get(x, np.float32(0.0)) + v)
    keep = [x for x in sorted(acc) if abs(acc[x]) > np.float32(tau)]
    g_idx = torch.tensor(keep, dtype=torch.int32)
    g_val = torch.from_numpy(np.array([acc[x] for x in keep], dtype=np.float32))
    return g_idx, g_val


def check_pair(fn, idx, val, counts, base, length, tau):
    """fn(idx, val, counts, base, length, tau) against brute(), in bits."""
    want_idx, want_val = brute(idx.cpu(), val.cpu(), counts, base, length, tau)
    g_idx, g_val = fn(idx, val, counts, base, length, tau)
    assert g_idx.dtype == torch.int32 and g_val.dtype == torch.float32
    assert g_idx.device == idx.device and g_val.device == idx.device
    assert torch.equal(g_idx.cpu(), want_idx)
    assert same_bits(g_val.cpu(), want_val)
    if g_idx.numel() > 1:
        assert bool((g_idx[1:] > g_idx[:-1]).all())
    return g_idx, g_val


# -- payloads ------------------------------------------------------------------

LAYOUTS = [[37], [0, 5, 0, 12, 1], [3, 0, 0, 7, 9, 1, 0, 11], [0, 0], [],
           [40] * 5]  # with "identical": every run has length P
OVERLAPS = ["disjoint", "identical", "random"]


def make_payload(seg_counts, overlap, base, length, seed, values="randn"):
    """Segments of ascending, duplicate-free indices drawn from
    [base - 3, base + length + 3), so some entries fall just outside on both
    sides.  The largest segment (when it has room) holds base - 1, base,
    base + length - 1 and base + length.  Returns (idx, val, counts)."""
    gen = torch.Generator().manual_seed(seed)
    pool = torch.arange(base - 3, base + length + 3)
    edges = torch.tensor([base - 1, base, base + length - 1, base + length])
    total = sum(seg_counts)
    assert total <= pool.numel() or overlap != "disjoint"

    def draw(c, source):
        return source[torch.randperm(source.numel(), generator=gen)[:c]]

    shuffled = draw(pool.numel(), pool)
    common = draw(max(seg_counts, default=0), pool).sort().values
    big = max(range(len(seg_counts)), key=lambda j: seg_counts[j], default=None)
    segs, off = [], 0
    for j, c in enumerate(seg_counts):
        if overlap == "disjoint":
            s = shuffled[off:off + c]
            off += c
        elif overlap == "identical":
            s = common[:c]
        else:
            s = draw(c, pool)
            if j == big and c >= 4:
                rest = pool[~torch.isin(pool, edges)]
                s = torch.cat([edges, draw(c - 4, rest)])
        segs.append(s.sort().values.to(torch.int32))
    idx = torch.cat(segs) if segs else torch.zeros(0, dtype=torch.int32)
    if values == "randn":
        val = torch.randn(total, generator=gen)
    elif values == "exact":  # multiples of 2^-8: every sum is order-free
        val = torch.randint(-512, 513, (total,), generator=gen).float() / 256
    else:
        raise AssertionError(values)
    return idx, val, list(seg_counts)


def pack_wire(idx, val, counts, wire_bf16):
    """[idx | val bits] per segment, the bf16 wire with its zero pad."""
    words, off = [], 0
    for c in counts:
        i, v = idx[off:off + c], val[off:off + c]
        off += c
        if wire_bf16:
            v = v.to(torch.bfloat16)
            if c % 2:
                v = torch.cat([v, v.new_zeros(1)])
        words += [i.view(torch.int32), v.view(torch.int32)]
    return torch.cat(words) if words else torch.zeros(0, dtype=torch.int32,
                                                      device=idx.device)


# one index, one contribution per segment (None: the segment is empty);
# want is the surviving value or None when the index is dropped
SUB = 1e-40  # subnormal in fp32
NAMED = {
    "big_cancels_first": ([1e8, -1e8, 1.0], 0.0, 1.0),
    "small_absorbed_then_cancel": ([1e8, 1.0, -1e8], 0.0, None),
    "v_minus_v": ([0.37, -0.37], 0.0, None),
    "two_below_tau_sum_above": ([0.3, 0.3], 0.5, 0.3 + 0.3),
    "two_above_tau_sum_below": ([0.7, -0.6], 0.5, None),
    "lone_negative_zero": ([None, -0.0, None], 0.0, None),
    "negative_zeros": ([-0.0, -0.0], 0.0, None),
    "subnormals": ([SUB, 2 * SUB, None, 4 * SUB], 0.0, "ieee"),
    "subnormal_cancel_to_subnormal": ([3 * SUB, -2 * SUB], 0.0, "ieee"),
    "nan": ([1.0, float("nan")], 0.0, None),
    "lone_nan": ([float("nan")], 0.0, None),
    "inf_minus_inf": ([float("inf"), 2.0, float("-inf")], 0.0, None),
    "inf_kept": ([float("inf"), 2.0], 0.5, float("inf")),
}


def named_payload(vals, at=5):
    counts = [0 if v is None else 1 for v in vals]
    present = [v for v in vals if v is not None]
    return (torch.full((len(present),), at, dtype=torch.int32),
            torch.tensor(present, dtype=torch.float32), counts)


def named_want(vals, want):
    if want != "ieee":
        return want
    s = np.float32(0.0)
    for v in vals:
        if v is not None:
            s = np.float32(s + np.float32(v))
    assert 0.0 < abs(float(s)) < 1.17549435e-38  # still subnormal, not flushed
    return float(s)


def check_named(fn, name, device="cpu"):
    vals, tau, want = NAMED[name]
    idx, val, counts = named_payload(vals)
    g_idx, g_val = check_pair(fn, idx.to(device), val.to(device), counts, 0, 16, tau)
    want = named_want(vals, want)
    if want is None:
        assert g_idx.numel() == 0
    else:
        assert g_idx.tolist() == [5]
        assert same_bits(g_val.cpu(), torch.tensor([want], dtype=torch.float32))


def all_named_in_one_payload():
    """Every named case at an index of its own (tau 0 and 0.5 cases kept
    apart by the caller): returns {tau: (idx, val, counts)}."""
    out = {}
    for tau in (0.0, 0.5):
        names = [n for n in NAMED if NAMED[n][1] == tau]
        P = max(len(NAMED[n][0]) for n in names)
        segs = [[] for _ in range(P)]
        for at, n in enumerate(names):
            for j, v in enumerate(NAMED[n][0]):
                if v is not None:
                    segs[j].append((3 * at + 1, v))
        idx = torch.tensor([x for s in segs for x, _ in s], dtype=torch.int32)
        val = torch.tensor([v for s in segs for _, v in s], dtype=torch.float32)
        out[tau] = (idx, val, [len(s) for s in segs])
    return out


# -- reference against brute force --------------------------------------------

@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("base", [0, 1000])
@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "-".join(map(str, l)) or "none")
def test_reference_matches_brute_force(layout, overlap, base, tau):
    length = 240 if overlap == "disjoint" else 60
    idx, val, counts = make_payload(layout, overlap, base, length, 31)
    if max(layout, default=0) >= 4 and overlap == "random":
        for x in (base - 1, base, base + length - 1, base + length):
            assert x in idx.tolist()
    check_pair(ops.reduce_segments, idx, val, counts, base, length, tau)
    check_pair(ref.reduce_segments, idx, val, counts, base, length, tau)


def test_identical_segments_make_runs_of_length_P():
    idx, val, counts = make_payload([40] * 5, "identical", 0, 60, 2)
    assert torch.unique(idx, return_counts=True)[1].tolist() == [5] * 40
    check_pair(ops.reduce_segments, idx, val, counts, 0, 60, 0.0)


def test_entries_outside_the_range_are_dropped():
    idx = torch.tensor([-1, 0, 9, 10, 2**31 - 1, -2**31, 0, 9], dtype=torch.int32)
    val = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.5, 0.25])
    g_idx, g_val = check_pair(ops.reduce_segments, idx[[5, 0, 1, 2, 3, 4, 6, 7]],
                              val[[5, 0, 1, 2, 3, 4, 6, 7]], [6, 2], 0, 10, 0.0)
    assert g_idx.tolist() == [0, 9] and g_val.tolist() == [2.5, 3.25]
    g_idx, _ = check_pair(ops.reduce_segments, idx[:4] + 1000, val[:4], [4],
                          1000, 10, 0.0)
    assert g_idx.tolist() == [1000, 1009]
    g_idx, _ = ops.reduce_segments(idx[:4], val[:4], [4], 0, 0, 0.0)
    assert g_idx.numel() == 0


@pytest.mark.parametrize("name", list(NAMED))
def test_named_value_cases(name):
    check_named(ops.reduce_segments, name)
    check_named(ref.reduce_segments, name)


def test_named_value_cases_in_one_payload():
    for tau, (idx, val, counts) in all_named_in_one_payload().items():
        check_pair(ops.reduce_segments, idx, val, counts, 0, 64, tau)


def test_summation_order_is_segment_order():
    # (a + b) + c and a + (b + c) differ here, and so do the permutations
    a, b, c = 1.0, 2.0 ** -24, 2.0 ** -24
    idx, val, counts = named_payload([a, b, c])
    _, v = ops.reduce_segments(idx, val, counts, 0, 16, 0.0)
    assert v.item() == 1.0  # each 2^-24 rounds away against 1.0
    idx, val, counts = named_payload([b, c, a])
    _, v = ops.reduce_segments(idx, val, counts, 0, 16, 0.0)
    assert v.item() == 1.0 + 2.0 ** -23


# -- wire form against pair form ------------------------------------------------

@pytest.mark.parametrize("wire_bf16", [False, True])
@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "-".join(map(str, l)) or "none")
def test_wire_form_equals_pair_form(layout, overlap, wire_bf16):
    length = 240 if overlap == "disjoint" else 60
    idx, val, counts = make_payload(layout, overlap, 1000, length, 41)
    buf = pack_wire(idx, val, counts, wire_bf16)
    if wire_bf16 and layout not in ([], [0, 0], [40] * 5):
        assert any(c % 2 for c in counts)  # pad half-words present
    u_idx, u_val = ops.unpack_segments(buf, counts, wire_bf16)
    assert torch.equal(u_idx, idx)
    for tau in (0.0, 0.5):
        want = check_pair(ops.reduce_segments, u_idx, u_val, counts, 1000,
                          length, tau)
        for fn in (ops.reduce_segments_wire, ref.reduce_segments_wire):
            g_idx, g_val = fn(buf, counts, wire_bf16, 1000, length, tau)
            assert g_idx.dtype == torch.int32
            assert torch.equal(g_idx, want[0]) and same_bits(g_val, want[1])


def test_wire_buffer_may_be_longer_than_the_counts_need():
    idx, val, counts = make_payload([5, 3], "random", 0, 20, 3)
    buf = torch.cat([pack_wire(idx, val, counts, True),
                     torch.full((7,), 0x7FC07FC0, dtype=torch.int32)])
    want = ops.reduce_segments_wire(buf[:-7].clone(), counts, True, 0, 20, 0.0)
    got = ops.reduce_segments_wire(buf, counts, True, 0, 20, 0.0)
    assert torch.equal(got[0], want[0]) and same_bits(got[1], want[1])


# -- argument checks ------------------------------------------------------------

def test_argument_errors():
    idx, val, counts = make_payload([5, 3], "random", 0, 20, 3)
    buf = pack_wire(idx, val, counts, False)
    for bad in (
        lambda: ops.reduce_segments(idx.long(), val, counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val.double(), counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(idx.reshape(2, 4), val, counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val.reshape(2, 4), counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val.to("meta"), counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val[:-1], counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val, [5, 2], 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val, [5, 4], 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val, [9, -1], 0, 20, 0.0),
        lambda: ops.reduce_segments(idx, val, counts, 0, 20, -0.5),
        lambda: ops.reduce_segments(idx, val, counts, 0, 20, float("nan")),
        lambda: ops.reduce_segments(idx, val, counts, 0, -1, 0.0),
        lambda: ops.reduce_segments_wire(buf.float(), counts, False, 0, 20, 0.0),
        lambda: ops.reduce_segments_wire(buf.reshape(2, 8), counts, False, 0, 20, 0.0),
        lambda: ops.reduce_segments_wire(buf, [5, 4], False, 0, 20, 0.0),
        lambda: ops.reduce_segments_wire(buf, [9, -1], False, 0, 20, 0.0),
        lambda: ops.reduce_segments_wire(buf, counts, False, 0, 20, -1.0),
        lambda: ops.reduce_segments_wire(buf, counts, False, 0, -3, 0.0),
    ):
        with pytest.raises(ValueError):
            bad()
    # the fp32 buffer is too short for nothing: the bf16 reading of it fits
    ops.reduce_segments_wire(buf, counts, True, 0, 20, 0.0)


# -- config / CLI ------------------------------------------------------------------

def test_flag_defaults_off_and_reaches_config():
    from oktopk_amd.train import build_argparser

    assert OkTopkConfig().device_reduce is False
    assert EngineConfig.preset("bert", device_reduce=True).oktopk.device_reduce
    assert build_argparser().parse_args([]).device_reduce is False
    assert build_argparser().parse_args(["--device-reduce"]).device_reduce is True


# -- engine: flag on against flag off ------------------------------------------------

N = 8192
DENSITY = 0.02
ITERS = 8
VARIANTS = {
    "plain": {},
    "chunked": {"pipeline_chunks": 2},
    "balanced": {"balanced_allgather": True},
}
CONFIGS = [(f"{name}/device_wire={dw}", dict(kw, device_wire=dw))
           for name, kw in VARIANTS.items() for dw in (False, True)]
CONFIGS.append(("plain/device_wire+device_round2",
                {"device_wire": True, "device_round2": True}))


def engine_grad(rank, it):
    """common(it) + 0.3 * noise(rank, it): the ranks' selections overlap
    heavily, so the reduce really sums."""
    common = torch.randn(N, generator=torch.Generator().manual_seed(911 + 17 * it))
    noise = torch.randn(
        N, generator=torch.Generator().manual_seed(7000 * rank + 13 * it + 5))
    return common + 0.3 * noise


def build_engine(flag, kw):
    import torch.distributed as dist

    from oktopk_amd import AllReducer, Comm

    return AllReducer(Comm(dist.group.WORLD), EngineConfig(
        compressor="oktopk", density=DENSITY, wire_dtype="fp32",
        oktopk=OkTopkConfig(
            dense_warmup_iters=0,
            local_threshold_recompute_interval=4,
            global_threshold_recompute_interval=3,
            region_repartition_interval=2,
            device_reduce=flag, **kw)))


def assert_same_state(on, off, where):
    assert sorted(off.states) == sorted(on.states)
    for name, st in on.states.items():
        ref_st = off.states[name]
        assert same_bits(st.residual, ref_st.residual), (where, name)
        assert st.tau_local == ref_st.tau_local, (where, name)
        assert st.tau_global == ref_st.tau_global, (where, name)
        if st.boundaries is None or ref_st.boundaries is None:
            assert st.boundaries is ref_st.boundaries, (where, name)
        else:
            assert torch.equal(st.boundaries, ref_st.boundaries), (where, name)


def engine_equivalence(rank, device, configs, world):
    """Worker: for every (label, OkTopkConfig kwargs) in `configs`, run the
    engine with device_reduce on and off over the same gradients and compare
    outputs, residuals, thresholds and boundaries in bits after every
    iteration.  A spy around the new op records how many ranks contributed
    to one index; the flagged engine must never reach a scatter-add."""
    from oktopk_amd import ops as eops

    if device == "cuda":
        torch.cuda.set_device(0)
    running = {"flag": None}
    most = []  # per call of the new op: the largest contributor count

    def contributors(idx, base, length):
        d = idx.long() - base
        d = d[(d >= 0) & (d < length)]
        most.append(int(torch.unique(d, return_counts=True)[1].max())
                    if d.numel() else 0)

    pair_op, wire_op = eops.reduce_segments, eops.reduce_segments_wire
    sa_op, usa_op = eops.scatter_add_, eops.unpack_scatter_add_

    def pair_spy(idx, val, counts, base, length, tau):
        assert running["flag"] is True
        contributors(idx, base, length)
        return pair_op(idx, val, counts, base, length, tau)

    def wire_spy(buf, counts, wire_bf16, base, length, tau):
        assert running["flag"] is True
        contributors(eops.unpack_segments(buf, counts, wire_bf16)[0], base, length)
        return wire_op(buf, counts, wire_bf16, base, length, tau)

    def sa_spy(*a):
        assert running["flag"] is False, "flagged engine reached scatter_add_"
        return sa_op(*a)

    def usa_spy(*a):
        assert running["flag"] is False, "flagged engine reached unpack_scatter_add_"
        return usa_op(*a)

    eops.reduce_segments, eops.reduce_segments_wire = pair_spy, wire_spy
    eops.scatter_add_, eops.unpack_scatter_add_ = sa_spy, usa_spy
    try:
        for label, kw in configs:
            off, on = build_engine(False, kw), build_engine(True, kw)
            del most[:]
            for it in range(ITERS):
                t = engine_grad(rank, it).to(device)
                running["flag"] = False
                a = off.run("w", t.clone())
                running["flag"] = True
                b = on.run("w", t.clone())
                running["flag"] = None
                assert same_bits(a, b), (label, it)
                assert_same_state(on, off, (label, it))
            assert any(st.tau_global > 0.0 for st in on.states.values())
            assert any(st.boundaries is not None for st in on.states.values())
            assert len(most) >= ITERS, (label, most)
            assert max(most) >= 2, (label, most)
            if world >= 3:
                assert max(most) >= 3, (label, most)
    finally:
        eops.reduce_segments, eops.reduce_segments_wire = pair_op, wire_op
        eops.scatter_add_, eops.unpack_scatter_add_ = sa_op, usa_op


@pytest.mark.parametrize("world", [2, 3, 4])
def test_engine_device_reduce_equals_scatter_add_composition(world):
    run_dist(engine_equivalence, world, args=("cpu", CONFIGS, world))
