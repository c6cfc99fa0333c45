"""HIP ordered-merge reduce (ops/csrc/reduce_merge.hip) against the CPU
reference, in the pair form and on both wires, in bits.

Sizes sit at the kernels' seams: 64 (wave), 256 (block / heads chunk), more
than 2048 * 256 merged entries (the grid-stride loop of the merge and a heads
chunk above one block), and the segment cap."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oktopk_amd import ops
from oktopk_amd.ops import reference as ref
from test_reduce_merge import (LAYOUTS, NAMED, OVERLAPS, all_named_in_one_payload,
                               check_named, make_payload, pack_wire, same_bits)


def offset_view(t):
    """Same contents at an odd element offset: 4-byte aligned, never 16."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:] = t
    return big[1:]


def assert_equal(got, want):
    assert got[0].is_cuda and got[0].dtype == torch.int32
    assert got[1].is_cuda and got[1].dtype == torch.float32
    assert torch.equal(got[0].cpu(), want[0])
    assert same_bits(got[1].cpu(), want[1])


def run_all_forms(idx, val, counts, base, length, tau, view=lambda t: t):
    """CPU payload -> the HIP op in the pair form, on the fp32 wire and on
    the bf16 wire, each against the CPU reference of the same form.  Returns
    the pair-form result."""
    want = ref.reduce_segments(idx, val, counts, base, length, tau)
    got = ops.reduce_segments(view(idx.cuda()), view(val.cuda()), counts, base,
                              length, tau)
    assert_equal(got, want)
    for wire_bf16 in (False, True):
        buf = pack_wire(idx, val, counts, wire_bf16)
        w_want = ref.reduce_segments_wire(buf, counts, wire_bf16, base, length, tau)
        if not wire_bf16:  # lossless: the pair form's result
            assert torch.equal(w_want[0], want[0]) and same_bits(w_want[1], want[1])
        w_got = ops.reduce_segments_wire(view(buf.cuda()), counts, wire_bf16,
                                         base, length, tau)
        assert_equal(w_got, w_want)
    return got


def spread_payload(counts, pool, base, seed, values="randn"):
    """Segment j: counts[j] ascending indices drawn from [base - 2,
    base - 2 + pool), independently per segment, so runs of every length up
    to P land anywhere in the merged order."""
    gen = torch.Generator().manual_seed(seed)
    segs = [(torch.randperm(pool, generator=gen)[:c].sort().values + base - 2)
            .to(torch.int32) for c in counts]
    total = sum(counts)
    if values == "randn":
        val = torch.randn(total, generator=gen)
    else:  # multiples of 2^-8: every sum is exact, so any order gives it
        val = torch.randint(-512, 513, (total,), generator=gen).float() / 256
    idx = torch.cat(segs) if segs else torch.zeros(0, dtype=torch.int32)
    return idx, val, list(counts)


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "-".join(map(str, l)) or "none")
def test_op_cases(layout, overlap, tau):
    length = 240 if overlap == "disjoint" else 60
    for base in (0, 1000):
        idx, val, counts = make_payload(layout, overlap, base, length, 31)
        run_all_forms(idx, val, counts, base, length, tau)


@pytest.mark.parametrize("name", list(NAMED))
def test_named_value_cases(name):
    check_named(ops.reduce_segments, name, device="cuda")
    vals, tau, _ = NAMED[name]
    counts = [0 if v is None else 1 for v in vals]
    present = torch.tensor([v for v in vals if v is not None])
    idx = torch.full((present.numel(),), 5, dtype=torch.int32)
    run_all_forms(idx, present, counts, 0, 16, tau)


def test_named_value_cases_in_one_payload():
    for tau, (idx, val, counts) in all_named_in_one_payload().items():
        run_all_forms(idx, val, counts, 0, 64, tau)


@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_runs_straddle_wave_and_block_boundaries(M):
    """Four segments over a pool of about M / 2 indices: runs of 2 to 4
    entries everywhere in the merged order, across position 64 and 256."""
    c = M // 4
    counts = [c, c, c, M - 3 * c]
    pool = max(M // 2, max(counts)) + 4
    idx, val, counts = spread_payload(counts, pool, 1000, 50 + M)
    if M >= 63:
        assert int(torch.unique(idx, return_counts=True)[1].max()) >= 3
    for tau in (0.0, 0.5):
        run_all_forms(idx, val, counts, 1000, pool - 4, tau)


def test_identical_sets_past_one_grid_stride_and_determinism():
    """M = 600 000 over P = 3 with identical index sets: every run has three
    entries, the merge grid-strides (2048 * 256 < M) and the heads chunk is
    above one block.  randn values, so the order of the three adds shows."""
    c = 200_000
    gen = torch.Generator().manual_seed(8)
    one = (torch.randperm(700_000, generator=gen)[:c].sort().values + 4998).to(torch.int32)
    idx = torch.cat([one, one, one])
    val = torch.randn(3 * c, generator=gen)
    counts = [c, c, c]
    want = ref.reduce_segments(idx, val, counts, 5000, 690_000, 0.25)
    # the reference's order is not the only one: another order gives other bits
    other = ref.reduce_segments(torch.cat([one, one, one]),
                                torch.cat([val[2 * c:], val[c:2 * c], val[:c]]),
                                counts, 5000, 690_000, 0.25)
    assert not (want[1].shape == other[1].shape and same_bits(want[1], other[1]))
    d_idx, d_val = idx.cuda(), val.cuda()
    first = ops.reduce_segments(d_idx, d_val, counts, 5000, 690_000, 0.25)
    assert_equal(first, want)
    again = ops.reduce_segments(d_idx, d_val, counts, 5000, 690_000, 0.25)
    assert torch.equal(again[0], first[0]) and same_bits(again[1], first[1])
    buf = pack_wire(idx, val, counts, False).cuda()
    for _ in range(2):
        w = ops.reduce_segments_wire(buf, counts, False, 5000, 690_000, 0.25)
        assert torch.equal(w[0], first[0]) and same_bits(w[1], first[1])


@pytest.mark.parametrize("wire_bf16", [False, True])
def test_offset_views(wire_bf16):
    """Inputs as views at an odd element offset: only 4-byte alignment may
    be assumed (the bf16 wire is read by 16-bit loads)."""
    idx, val, counts = spread_payload([333, 0, 1025, 7], 1500, 0, 77)
    run_all_forms(idx, val, counts, 0, 1490, 0.3, view=offset_view)


def test_segment_cap_and_fallback():
    """P at the device cap runs the kernels; one more falls back to the
    reference on the same device.  Exact values: the reference's atomics on
    the GPU then give the same bits in any order."""
    from oktopk_amd import _hip_ops

    cap = ops.reduce_max_segments()
    assert cap == _hip_ops.reduce_max_segments()
    assert 2 <= cap <= _hip_ops.wire_max_segments()
    probe = torch.zeros(1, device="cuda")
    assert ops._reduce_backend(probe, cap) is _hip_ops
    assert ops._reduce_backend(probe, cap + 1) is ref
    for P in (cap, cap + 1):
        counts = [(j * 7) % 23 for j in range(P)]
        idx, val, counts = spread_payload(counts, 40, 100, P, values="exact")
        assert int(torch.unique(idx, return_counts=True)[1].max()) > 8
        for tau in (0.0, 1.0):
            got = run_all_forms(idx, val, counts, 100, 36, tau)
            assert got[0].numel() > 0
    with pytest.raises(RuntimeError):  # the binding itself refuses
        _hip_ops.reduce_segments(idx.cuda(), val.cuda(), counts, 100, 36, 0.0)


def test_empty_payloads():
    e_i, e_v = torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    for counts in ([], [0], [0, 0, 0]):
        got = run_all_forms(e_i, e_v, counts, 10, 100, 0.0)
        assert got[0].numel() == 0 and got[1].numel() == 0
    idx, val, counts = spread_payload([300, 300], 500, 0, 4)
    got = run_all_forms(idx, val, counts, 0, 0, 0.0)  # an empty region
    assert got[0].numel() == 0


def test_every_entry_filtered_out():
    idx, val, counts = spread_payload([300, 280, 310], 500, 0, 6)
    for base, length, tau in ((1000, 500, 0.0),      # all below the range
                              (-2000, 500, 0.0),     # all above it
                              (0, 500, 1e30)):       # none above tau
        got = run_all_forms(idx, val, counts, base, length, tau)
        assert got[0].numel() == 0
    # exact cancellation everywhere
    one, v = idx[:300], val[:300]
    got = run_all_forms(torch.cat([one, one]), torch.cat([v, -v]), [300, 300],
                        -5, 600, 0.0)
    assert got[0].numel() == 0


def test_force_torch_env_selects_the_reference(monkeypatch):
    monkeypatch.setattr(ops, "_FORCE_TORCH", True)
    assert ops._reduce_backend(torch.zeros(1, device="cuda"), 2) is ref
    idx, val, counts = spread_payload([50, 60], 90, 0, 9, values="exact")
    want = ref.reduce_segments(idx, val, counts, 0, 86, 0.0)
    got = ops.reduce_segments(idx.cuda(), val.cuda(), counts, 0, 86, 0.0)
    assert_equal(got, want)


def test_argument_errors():
    idx, val, counts = spread_payload([5, 3], 30, 0, 3)
    d_idx, d_val = idx.cuda(), val.cuda()
    buf = pack_wire(idx, val, counts, False).cuda()
    for bad in (
        lambda: ops.reduce_segments(d_idx.long(), d_val, counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(d_idx, d_val.double(), counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(d_idx, val, counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(d_idx, d_val[:-1], counts, 0, 20, 0.0),
        lambda: ops.reduce_segments(d_idx, d_val, [5, 4], 0, 20, 0.0),
        lambda: ops.reduce_segments(d_idx, d_val, [9, -1], 0, 20, 0.0),
        lambda: ops.reduce_segments(d_idx, d_val, counts, 0, 20, -0.5),
        lambda: ops.reduce_segments(d_idx, d_val, counts, 0, -1, 0.0),
        lambda: ops.reduce_segments_wire(buf.float(), counts, False, 0, 20, 0.0),
        lambda: ops.reduce_segments_wire(buf, [5, 4], False, 0, 20, 0.0),
        lambda: ops.reduce_segments_wire(buf, counts, False, 0, 20, -1.0),
    ):
        with pytest.raises(ValueError):
            bad()
