"""Sparse wire codec on the GPU: the HIP kernels of ops/csrc/wire_codec.hip
against the CPU reference (ops/reference.py), and the device_wire engine
path against the host path with both ranks computing on cuda:0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import run_dist
from oktopk_amd.ops import reference as R

from test_wire_codec import SPECIAL_BITS, boundary_tables, selection

SIZES = [0, 1, 63, 64, 65, 255, 257, 4097, 600_001]  # last: > 2048 x 256
PARTS = [1, 2, 3, 8, 64, 256]
WIRES = [False, True]


def hip():
    from oktopk_amd import _hip_ops

    return _hip_ops


def dirty(words):
    """Leave a freed block of -1 words for the caching allocator to hand
    to the next same-sized allocation: a word (or pad half-word) the pack
    kernel fails to write then shows up as a mismatch."""
    if words:
        junk = torch.full((words,), -1, dtype=torch.int32, device="cuda")
        del junk


def cap_words(m, P, wire_bf16):
    return m + (m + P) // 2 if wire_bf16 else 2 * m


def check_pack(idx, val, bounds, wire_bf16, tag):
    want, want_counts = R.pack_regions(idx, val, bounds, wire_bf16)
    gi, gv = idx.cuda(), val.cuda()
    dirty(cap_words(idx.numel(), bounds.numel() - 1, wire_bf16))
    got, counts = hip().pack_regions(gi, gv, bounds, wire_bf16)
    assert list(counts) == want_counts, tag
    assert got.is_cuda and got.dtype == torch.int32
    assert torch.equal(got.cpu(), want), tag


@pytest.mark.parametrize("P", PARTS)
@pytest.mark.parametrize("m", SIZES)
def test_pack_regions_matches_reference(m, P):
    n = max(3 * m, 2 * P, 16)
    idx, val = selection(m, n, seed=m % 1009 + P)
    bounds = boundary_tables(P, idx, n)["uniform"]
    for wire_bf16 in WIRES:
        check_pack(idx, val, bounds, wire_bf16, (m, P, wire_bf16))


@pytest.mark.parametrize("P,m", [(2, 65), (3, 11), (8, 257), (64, 4097), (256, 4097)])
def test_pack_regions_boundary_cases(P, m):
    n = 4 * m
    idx, val = selection(m, n, seed=P + m)
    for name, bounds in boundary_tables(P, idx, n).items():
        for wire_bf16 in WIRES:
            check_pack(idx, val, bounds, wire_bf16, (name, wire_bf16))


def test_pack_regions_odd_segment_counts():
    """Every segment odd: each carries a pad half-word that must be zero."""
    counts = [1, 3, 5, 63, 65, 255, 257, 1]
    idx = torch.arange(sum(counts), dtype=torch.int32)
    val = torch.full((sum(counts),), -1.5)
    b = [0]
    for c in counts:
        b.append(b[-1] + c)
    bounds = torch.tensor(b, dtype=torch.int64)
    dirty(cap_words(idx.numel(), len(counts), True))
    got, got_counts = hip().pack_regions(idx.cuda(), val.cuda(), bounds, True)
    assert list(got_counts) == counts
    want, _ = R.pack_regions(idx, val, bounds, True)
    assert torch.equal(got.cpu(), want)
    off = 0
    for c in counts:
        words = c + (c + 1) // 2
        assert want[off + c:off + words].view(torch.int16)[c] == 0
        off += words


@pytest.mark.parametrize("wire_bf16", WIRES)
def test_pack_regions_offset_views(wire_bf16):
    """idx / val taken as [1:] views: 4-byte alignment only."""
    m, P = 4097, 8
    idx, val = selection(m + 1, 4 * m, seed=7)
    gi, gv = idx.cuda()[1:], val.cuda()[1:]
    assert gi.data_ptr() % 16 == 4 and gv.data_ptr() % 16 == 4
    bounds = boundary_tables(P, idx[1:], 4 * m)["uniform"]
    want, want_counts = R.pack_regions(idx[1:], val[1:], bounds, wire_bf16)
    dirty(cap_words(m, P, wire_bf16))
    got, counts = hip().pack_regions(gi, gv, bounds, wire_bf16)
    assert list(counts) == want_counts
    assert torch.equal(got.cpu(), want)


def test_bf16_conversion_bit_equal_to_torch():
    g = torch.Generator().manual_seed(11)
    bits = torch.tensor(SPECIAL_BITS, dtype=torch.int64).to(torch.int32)
    val = torch.cat([bits.view(torch.float32), torch.randn(5000, generator=g),
                     torch.randn(5000, generator=g) * 1e-30,
                     torch.randn(5000, generator=g) * 1e30])
    m = val.numel()
    idx = torch.arange(m, dtype=torch.int32)
    bounds = torch.tensor([0, m], dtype=torch.int64)
    dirty(cap_words(m, 1, True))
    buf, counts = hip().pack_regions(idx.cuda(), val.cuda(), bounds, True)
    assert list(counts) == [m]
    got = buf.cpu()[m:].view(torch.int16)[:m]
    want = val.to(torch.bfloat16).view(torch.int16)
    assert torch.equal(got, want)


def test_bf16_conversion_nan_stays_nan():
    bits = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF,
            0x7F80FFFF, 0x7FBFFFFF]
    val = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert torch.isnan(val).all()
    m = val.numel()
    idx = torch.arange(m, dtype=torch.int32)
    bounds = torch.tensor([0, m], dtype=torch.int64)
    buf, _ = hip().pack_regions(idx.cuda(), val.cuda(), bounds, True)
    _, out = hip().unpack_segments(buf, [m], True)
    assert torch.isnan(out).all()


def wire_payload(P, m, base, size, seed, wire_bf16, quantise=False, same=False):
    """P senders' segments for one owned region [base, base + size), built
    with the CPU reference."""
    g = torch.Generator().manual_seed(seed)
    segs, counts = [], []
    for j in range(P):
        c = m if (same or j % 2 == 0) else m // 2
        i = torch.arange(c) if same else torch.randperm(size, generator=g)[:c].sort().values
        v = torch.randn(c, generator=g)
        if quantise:  # multiples of 2^-8, |v| < 256
            v = (v * 64).round().clamp(-65535, 65535) / 256
        b, _ = R.pack_regions((i + base).to(torch.int32), v,
                              torch.tensor([0, base + size], dtype=torch.int64),
                              wire_bf16)
        segs.append(b)
        counts.append(c)
    return torch.cat(segs), counts


@pytest.mark.parametrize("P", PARTS)
@pytest.mark.parametrize("m", SIZES)
def test_unpack_segments_matches_reference(m, P):
    m = min(m, 4097) if P > 8 else m  # P x m entries: keep the payload small
    for wire_bf16 in WIRES:
        buf, counts = wire_payload(P, m, 5, max(m, 1) + 3, m + P, wire_bf16)
        want_i, want_v = R.unpack_segments(buf, counts, wire_bf16)
        got_i, got_v = hip().unpack_segments(buf.cuda(), counts, wire_bf16)
        assert got_i.dtype == torch.int32 and got_v.dtype == torch.float32
        assert torch.equal(got_i.cpu(), want_i)
        assert torch.equal(got_v.cpu(), want_v)


@pytest.mark.parametrize("wire_bf16", WIRES)
@pytest.mark.parametrize("m", SIZES)
def test_unpack_scatter_add_two_senders_bit_equal(m, wire_bf16):
    """P = 2: a slot gets at most two contributions, so the order of the
    atomic adds cannot change the sum."""
    base, size = 12345, 2 * m + 9
    buf, counts = wire_payload(2, m, base, size, m + 1, wire_bf16)
    want = R.unpack_scatter_add_(torch.zeros(size), buf, counts, base, wire_bf16)
    dest = torch.zeros(size, device="cuda")
    out = hip().unpack_scatter_add_(dest, buf.cuda(), counts, base, wire_bf16)
    assert out.data_ptr() == dest.data_ptr()
    assert torch.equal(dest.cpu(), want)


@pytest.mark.parametrize("wire_bf16", WIRES)
def test_unpack_scatter_add_eight_senders_same_slots(wire_bf16):
    P, slots, base, size = 8, 1000, 777, 1500
    # exactly summable values: any order gives the same bits
    buf, counts = wire_payload(P, slots, base, size, 1, wire_bf16,
                               quantise=True, same=True)
    want = R.unpack_scatter_add_(torch.zeros(size), buf, counts, base, wire_bf16)
    dest = torch.zeros(size, device="cuda")
    hip().unpack_scatter_add_(dest, buf.cuda(), counts, base, wire_bf16)
    assert torch.equal(dest.cpu(), want)
    assert dest[slots:].abs().sum().item() == 0.0

    # randn values against fp64: each of the P-1 roundings of a slot's
    # running sum is at most half an ulp of a partial sum, and every
    # partial sum is bounded by sum|v_i|  ->  (P-1) * 2^-24 * sum|v_i|
    buf, counts = wire_payload(P, slots, base, size, 2, wire_bf16, same=True)
    idx, val = R.unpack_segments(buf, counts, wire_bf16)
    ref = torch.zeros(size, dtype=torch.float64)
    ref.index_add_(0, idx.long() - base, val.double())
    mag = torch.zeros(size, dtype=torch.float64)
    mag.index_add_(0, idx.long() - base, val.double().abs())
    bound = (P - 1) * 2.0 ** -24 * mag
    dest = torch.zeros(size, device="cuda")
    hip().unpack_scatter_add_(dest, buf.cuda(), counts, base, wire_bf16)
    err = (dest.cpu().double() - ref).abs()
    print(f"max err {err.max().item():.3e}  min slack "
          f"{(bound - err)[:slots].min().item():.3e}")
    assert (err <= bound).all()


def test_empty_and_all_empty_segments():
    bounds = torch.tensor([0, 10, 20, 30], dtype=torch.int64)
    e_i = torch.empty(0, dtype=torch.int32, device="cuda")
    e_v = torch.empty(0, device="cuda")
    for wire_bf16 in WIRES:
        buf, counts = hip().pack_regions(e_i, e_v, bounds, wire_bf16)
        assert buf.numel() == 0 and buf.is_cuda and list(counts) == [0, 0, 0]
        i, v = hip().unpack_segments(buf, [0, 0, 0], wire_bf16)
        assert i.numel() == 0 and v.numel() == 0
        assert i.dtype == torch.int32 and v.dtype == torch.float32
        dest = torch.ones(7, device="cuda")
        hip().unpack_scatter_add_(dest, buf, [0, 0, 0], 0, wire_bf16)
        assert torch.equal(dest.cpu(), torch.ones(7))


def test_more_segments_than_the_kernels_take_fall_back():
    from oktopk_amd import ops

    P = hip().wire_max_segments() + 1
    assert hip().wire_max_segments() >= 256
    m, n = 3000, 4 * (hip().wire_max_segments() + 1)
    idx, val = selection(m, n, seed=3)
    bounds = boundary_tables(P, idx, n)["uniform"]
    want, want_counts = R.pack_regions(idx, val, bounds, True)
    got, counts = ops.pack_regions(idx.cuda(), val.cuda(), bounds, True)
    assert got.is_cuda and counts == want_counts
    assert torch.equal(got.cpu(), want)
    i, v = ops.unpack_segments(got, counts, True)
    assert i.is_cuda and torch.equal(i.cpu(), idx)
    dest = torch.zeros(n, device="cuda")
    ops.unpack_scatter_add_(dest, got, counts, 0, True)
    assert torch.equal(dest.cpu()[idx.long()], val.bfloat16().float())


# -- engine equivalence: ranks share cuda:0, gloo transport ---------------

N = 200_000
DENSITY = 0.01


def _grad(rank, it, quantise):
    g = torch.Generator().manual_seed(1000 * rank + it)
    t = torch.randn(N, generator=g)
    if quantise:  # multiples of 2^-8: every sum below is exact in any order
        t = (t * 256).round() / 256
    return t


def _engine_equivalence_gpu(rank, wires, quantise):
    import torch.distributed as dist

    from oktopk_amd import AllReducer, Comm, EngineConfig
    from oktopk_amd.config import OkTopkConfig

    torch.cuda.set_device(0)

    def build(wire, device_wire):
        return AllReducer(Comm(dist.group.WORLD), EngineConfig(
            compressor="oktopk", density=DENSITY, wire_dtype=wire,
            oktopk=OkTopkConfig(dense_warmup_iters=1,
                                region_repartition_interval=3,
                                device_wire=device_wire)))

    for wire in wires:
        host, dev = build(wire, False), build(wire, True)
        # it 0 dense warm-up, it 1 exact global recompute (tau_global unset),
        # it 3 repartition
        for it in range(6):
            t = _grad(rank, it, quantise).cuda()
            a = host.run("w", t.clone())
            b = dev.run("w", t.clone())
            assert a.is_cuda and b.is_cuda
            assert torch.equal(a, b), (wire, it, (a - b).abs().max().item())
            assert torch.equal(host.states["w"].residual,
                               dev.states["w"].residual), (wire, it)
        assert host.states["w"].tau_global == dev.states["w"].tau_global > 0.0
        if quantise:
            continue
        # the stage pipeline (run_many) takes the same ops through
        # _oktopk_pipeline: a batch of 2 tensors
        host, dev = build(wire, False), build(wire, True)
        for it in range(4):
            ta = [_grad(rank, 10 * s + it, False).cuda() for s in range(2)]
            tb = [t.clone() for t in ta]
            host.run_many([(f"b{s}", ta[s], None) for s in range(2)])
            dev.run_many([(f"b{s}", tb[s], None) for s in range(2)])
            for s in range(2):
                assert torch.equal(ta[s], tb[s]), (wire, it, s)
                assert torch.equal(host.states[f"b{s}"].residual,
                                   dev.states[f"b{s}"].residual), (wire, it, s)


def test_gpu_world2_device_wire_equals_host_path():
    run_dist(_engine_equivalence_gpu, 2, args=(("fp32", "bf16"), False))


def test_gpu_world3_device_wire_equals_host_path_exact_sums():
    run_dist(_engine_equivalence_gpu, 3, args=(("fp32", "bf16"), True))
