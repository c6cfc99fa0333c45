"""HIP round-2 tail (ops/csrc/round2_tail.hip) against the torch references
on the same device.  Outputs, tau and the WHOLE residual are compared in
bits, so a stray store anywhere in the residual fails the test.

Sizes sit at the kernels' seams: 64 (wave), 512 (wave sub-chunk of the
count / write passes), 2048 (block chunk), and several blocks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oktopk_amd import ops
from oktopk_amd.ops import reference as ref
from test_round2_tail import K_OF, make_case, same_bits, wire_case

SIZES = [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 20_000]


def cuda(*ts):
    return tuple(t.cuda() for t in ts)


def offset_view(t):
    """Same contents at an odd element offset: 4-byte aligned, never 16."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:] = t
    v = big[1:]
    assert v.data_ptr() % 16 != 0 or t.numel() == 0
    return v


def run_both(residual, idx, k, pair=None, wire=None):
    """HIP op and reference on clones of the same device residual; asserts
    bit equality of everything and returns the HIP result."""
    r_hip, r_ref = residual.clone(), residual.clone()
    if wire is not None:
        buf, counts, bf = wire
        got = ops.round2_tail_wire_(r_hip, idx, buf, counts, bf, k)
        want = ref.round2_tail_wire_(r_ref, idx, buf, counts, bf, k)
    else:
        got = ops.round2_tail_(r_hip, idx, pair[0], pair[1], k)
        want = ref.round2_tail_(r_ref, idx, pair[0], pair[1], k)
    assert got[0].is_cuda and got[0].dtype == torch.int32
    assert got[1].is_cuda and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0])
    assert same_bits(got[1], want[1])
    assert got[2] == want[2] and (got[2] is None or isinstance(got[2], float))
    assert same_bits(r_hip, r_ref)
    return got, r_hip


def ks_for(S):
    out = []
    for name in K_OF:
        k = K_OF[name](S)
        if k is None or k >= 1:
            out.append(k)
    return out


@pytest.mark.parametrize("S", SIZES)
def test_pair_form_sizes(S):
    n = 4 * S + 7
    for values in ("randn", "few"):
        for m in sorted({0, 1, S}):
            residual, idx, all_idx, all_val = cuda(
                *make_case(n, S, m, 100 + S, values=values))
            for k in ks_for(S):
                (g_idx, g_val, tau), res = run_both(
                    residual, idx, k, pair=(all_idx, all_val))
                if k is None:  # returned as they are, no copy
                    assert g_idx is all_idx and g_val is all_val and tau is None
                else:
                    assert g_idx.numel() == min(k, S) and tau is not None
                if m == 0:
                    assert same_bits(res, residual)


@pytest.mark.parametrize("overlap", ["identical", "disjoint"])
def test_pair_form_identical_and_disjoint_lists(overlap):
    S = 2049
    residual, idx, all_idx, all_val = cuda(
        *make_case(3 * S, S, S // 2, 9, overlap=overlap))
    for k in (None, 1, 700, S, S + 5):
        (g_idx, _, _), res = run_both(residual, idx, k, pair=(all_idx, all_val))
        zeroed = int((res == 0).sum())
        assert zeroed == (g_idx.numel() if overlap == "identical" else 0)


def test_one_magnitude_tie_rule_decides_everything():
    S = 5000
    residual, idx, all_idx, all_val = cuda(
        *make_case(3 * S, S, S, 21, "identical", "one_magnitude"))
    for k in (1, 63, 64, 65, 512, 513, 2048, 2049, 4999, S):
        (g_idx, _, tau), _ = run_both(residual, idx, k, pair=(all_idx, all_val))
        assert torch.equal(g_idx, all_idx[:k]) and tau == 0.75


def test_tie_class_across_sub_chunk_and_block_boundary():
    """Ties at positions 500..530 (across the wave sub-chunk seam at 512)
    and 2040..2060 (across the block seam at 2048), 100 larger entries;
    `need` ends before, at and after each seam."""
    S = 3000
    gen = torch.Generator().manual_seed(33)
    val = torch.rand(S, generator=gen) * 0.4 + 0.05
    big = torch.randperm(S, generator=gen)
    ties = list(range(500, 531)) + list(range(2040, 2061))
    big = [p for p in big.tolist() if p not in set(ties)][:100]
    val[big] = torch.rand(100, generator=gen) + 2.0
    val[ties] = 1.0
    val *= (torch.randint(0, 2, (S,), generator=gen) * 2 - 1).float()
    all_idx = torch.arange(S, dtype=torch.int32) * 3 + 1
    idx = all_idx[::2].clone()
    residual = torch.full((3 * S + 5,), 2.5)
    residual, idx, all_idx, val = cuda(residual, idx, all_idx, val)
    for need in (1, 11, 12, 13, 30, 31, 32, 38, 39, 40, 41, 51, 52):
        (g_idx, g_val, tau), _ = run_both(residual, idx, 100 + need,
                                          pair=(all_idx, val))
        assert tau == 1.0
        picked = (g_val.abs() == 1.0).nonzero().reshape(-1)
        assert picked.numel() == need
        want = torch.tensor(ties[:need], dtype=torch.int32) * 3 + 1
        assert torch.equal(g_idx[picked].cpu(), want)


def test_signed_zeros_and_credit_sign():
    all_idx = torch.arange(0, 200, 2, dtype=torch.int32)
    all_val = torch.zeros(100)
    all_val[1::2] = -0.0
    all_val[50] = 3.0
    idx = torch.arange(0, 200, 4, dtype=torch.int32)
    residual = torch.full((200,), -1.5)
    residual, idx, all_idx, all_val = cuda(residual, idx, all_idx, all_val)
    for k in (None, 1, 2, 40, 100):
        _, res = run_both(residual, idx, k, pair=(all_idx, all_val))
        assert not bool(torch.signbit(res[res == 0]).any())  # +0.0 only


def test_out_of_range_matches_are_dropped():
    all_idx = torch.tensor([2, 7, 40, 90, 2_000_000_000], dtype=torch.int32)
    all_val = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    idx = torch.tensor([7, 40, 90, 2_000_000_000], dtype=torch.int32)
    residual = torch.ones(40)
    guard = torch.ones(64)  # a neighbouring allocation must stay untouched
    residual, idx, all_idx, all_val, guard = cuda(residual, idx, all_idx,
                                                  all_val, guard)
    for k in (None, 5, 4):  # 7 is selected and in range; 40, 90, 2e9 are not
        _, res = run_both(residual, idx, k, pair=(all_idx, all_val))
        assert res[7] == 0.0 and int((res == 0).sum()) == 1
    _, res = run_both(residual, idx, 3, pair=(all_idx, all_val))  # 7 not selected
    assert int((res == 0).sum()) == 0
    assert bool((guard == 1).all())


@pytest.mark.parametrize("wire_bf16", [False, True])
@pytest.mark.parametrize("segs", [
    [1], [65], [0, 513, 0], [700, 1, 1348], [2049],
    [3, 0, 0, 777, 901, 1, 0, 366], [2500] * 8, [0, 0, 0],
])
def test_wire_form(wire_bf16, segs):
    S = sum(segs)
    # bf16: a handful of magnitudes, so the k-th one ties by construction
    residual, idx, buf, counts = cuda_wire(
        wire_case(4 * S + 9, segs, max(S - 3, 0), 300 + len(segs), wire_bf16,
                  "few" if wire_bf16 else "randn"))
    all_idx, all_val = ops.unpack_segments(buf, counts, wire_bf16)
    for k in ks_for(S) if S else (None, 1, 9):
        r_pair = residual.clone()
        want = ops.round2_tail_(r_pair, idx, all_idx, all_val, k)
        (g_idx, g_val, tau), res = run_both(residual, idx, k,
                                            wire=(buf, counts, wire_bf16))
        assert torch.equal(g_idx, want[0]) and same_bits(g_val, want[1])
        assert tau == want[2] and same_bits(res, r_pair)
        if k is None:
            assert torch.equal(g_idx, all_idx) and same_bits(g_val, all_val)


def cuda_wire(case):
    residual, idx, buf, counts = case
    return residual.cuda(), idx.cuda(), buf.cuda(), counts


@pytest.mark.parametrize("wire_bf16", [False, True])
def test_offset_views(wire_bf16):
    """buf, idx, residual (and the pair lists) as views at an odd element
    offset: only 4-byte alignment may be assumed."""
    segs = [333, 0, 1025, 7]
    S = sum(segs)
    residual, idx, buf, counts = cuda_wire(
        wire_case(4 * S, segs, S, 77, wire_bf16,
                  "few" if wire_bf16 else "randn"))
    all_idx, all_val = ops.unpack_segments(buf, counts, wire_bf16)
    r_o, i_o, b_o = offset_view(residual), offset_view(idx), offset_view(buf)
    ai_o, av_o = offset_view(all_idx), offset_view(all_val)
    for k in (None, 1, 400, S - 1, S + 5):
        (w_idx, w_val, w_tau), w_res = run_both(r_o, i_o, k,
                                                wire=(b_o, counts, wire_bf16))
        (p_idx, p_val, p_tau), p_res = run_both(r_o, i_o, k, pair=(ai_o, av_o))
        (a_idx, a_val, a_tau), a_res = run_both(residual, idx, k,
                                                pair=(all_idx, all_val))
        for x_idx, x_val, x_tau, x_res in ((w_idx, w_val, w_tau, w_res),
                                           (p_idx, p_val, p_tau, p_res)):
            assert torch.equal(x_idx, a_idx) and same_bits(x_val, a_val)
            assert x_tau == a_tau and same_bits(x_res, a_res)


def test_more_segments_than_the_tables_hold():
    """Beyond wire_max_segments the torch reference runs on the device."""
    from oktopk_amd import _hip_ops

    P = _hip_ops.wire_max_segments() + 1
    segs = [(j % 3 == 0) * 2 for j in range(P)]
    S = sum(segs)
    residual, idx, buf, counts = cuda_wire(wire_case(4 * S, segs, S, 5, True, "few"))
    for k in (None, S // 2):
        (g_idx, _, _), _ = run_both(residual, idx, k, wire=(buf, counts, True))
        assert g_idx.is_cuda and g_idx.numel() == (S if k is None else k)


def test_argument_errors():
    residual, idx, all_idx, all_val = cuda(*make_case(100, 20, 10, 2))
    for bad in (
        lambda: ops.round2_tail_(residual, idx, all_idx, all_val, 0),
        lambda: ops.round2_tail_(residual, idx.long(), all_idx, all_val),
        lambda: ops.round2_tail_(residual, idx, all_idx, all_val.double()),
        lambda: ops.round2_tail_(residual, idx, all_idx, all_val[:-1], 3),
        lambda: ops.round2_tail_(residual, idx.cpu(), all_idx, all_val),
        lambda: ops.round2_tail_wire_(residual, idx, all_idx, [21], False),
    ):
        with pytest.raises(ValueError):
            bad()
