"""ops.sparse_merge_topk, reference backend (CPU), against a dense oracle:
scatter both lists into a small index space with a presence mask, then a
stable descending sort of |v| over the present entries."""
import pytest
import torch

from oktopk_amd import ops

N = 1 << 20
LENGTHS = [0, 1, 63, 64, 65, 1000, 110_000]


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int32)


def make_lists(la: int, lb: int, overlap: float, mode: str, seed: int):
    """Two ascending unique index lists sharing round(overlap * min) entries.
    mode: "randn" | "quant" (few value levels, ties) | "cancel" (b = -a on
    the shared indices)."""
    g = torch.Generator().manual_seed(seed)
    shared = int(round(overlap * min(la, lb)))
    perm = torch.randperm(N, generator=g)
    common = perm[:shared]
    a_idx = torch.cat([common, perm[shared:la]]).sort().values
    b_idx = torch.cat([common, perm[la:la + lb - shared]]).sort().values

    def values(m):
        v = torch.randn(m, generator=g)
        return torch.round(v * 2) / 2 if mode == "quant" else v

    a_val, b_val = values(la), values(lb)
    if mode == "cancel" and shared:
        dense_a = torch.zeros(N)
        dense_a[a_idx] = a_val
        hit = torch.isin(b_idx, common)
        b_val[hit] = -dense_a[b_idx[hit]]
    return a_idx.to(torch.int32), a_val, b_idx.to(torch.int32), b_val


def dense_oracle(a_idx, a_val, b_idx, b_val, k):
    dense = torch.zeros(N)
    present = torch.zeros(N, dtype=torch.bool)
    for i, v in ((a_idx, a_val), (b_idx, b_val)):
        dense[i.long()] += v
        present[i.long()] = True
    u_idx = present.nonzero().reshape(-1)
    u_val = dense[u_idx]
    k = min(k, u_idx.numel())
    order = torch.sort(u_val.abs(), descending=True, stable=True).indices[:k]
    keep = torch.sort(order).values
    return u_idx[keep].to(torch.int32), u_val[keep], u_idx.numel()


def ks_for(union: int):
    return sorted({1, max(1, union // 3), max(1, union), union + 17})


def check(a_idx, a_val, b_idx, b_val):
    _, _, union = dense_oracle(a_idx, a_val, b_idx, b_val, 1)
    inputs = [x.clone() for x in (a_idx, a_val, b_idx, b_val)]
    for k in ks_for(union):
        o_idx, o_val, _ = dense_oracle(a_idx, a_val, b_idx, b_val, k)
        idx, val = ops.sparse_merge_topk(a_idx, a_val, b_idx, b_val, k)
        assert idx.dtype == torch.int32 and val.dtype == torch.float32
        assert idx.numel() == min(k, union)
        assert torch.equal(idx, o_idx)
        # the dense scatter turns a lone -0.0 into +0.0; values compare equal
        assert torch.equal(val, o_val)
    for x, y in zip(inputs, (a_idx, a_val, b_idx, b_val)):
        assert torch.equal(bits(x), bits(y))  # inputs untouched


@pytest.mark.parametrize("la", LENGTHS)
@pytest.mark.parametrize("lb", [0, 1, 64, 65, 1000])
@pytest.mark.parametrize("overlap", [0.0, 0.5, 1.0])
def test_merge_lengths_and_overlap(la, lb, overlap):
    check(*make_lists(la, lb, overlap, "randn", seed=la * 7 + lb))


@pytest.mark.parametrize("overlap", [0.0, 0.5, 1.0])
def test_merge_long_lists(overlap):
    check(*make_lists(110_000, 110_000, overlap, "randn", seed=5))


@pytest.mark.parametrize("la,lb", [(65, 64), (1000, 1000), (110_000, 1000)])
@pytest.mark.parametrize("overlap", [0.5, 1.0])
def test_merge_exact_cancellation_stays_in_union(la, lb, overlap):
    a_idx, a_val, b_idx, b_val = make_lists(la, lb, overlap, "cancel", seed=9)
    check(a_idx, a_val, b_idx, b_val)
    union = torch.unique(torch.cat([a_idx, b_idx])).numel()
    idx, val = ops.sparse_merge_topk(a_idx, a_val, b_idx, b_val, union)
    assert idx.numel() == union  # zero sums are entries, not holes
    assert int((val == 0).sum()) >= int(round(overlap * min(la, lb)))


@pytest.mark.parametrize("la,lb", [(63, 65), (1000, 1000), (110_000, 110_000)])
@pytest.mark.parametrize("overlap", [0.0, 0.5, 1.0])
def test_merge_quantised_values_tie_by_lowest_index(la, lb, overlap):
    check(*make_lists(la, lb, overlap, "quant", seed=13))


def test_merge_small_by_hand():
    a_idx = torch.tensor([2, 5, 9], dtype=torch.int32)
    a_val = torch.tensor([1.0, -4.0, 2.0])
    b_idx = torch.tensor([5, 7, 9, 11], dtype=torch.int32)
    b_val = torch.tensor([4.0, 2.0, 1.0, -2.0])
    # union: 2:1, 5:0, 7:2, 9:3, 11:-2
    idx, val = ops.sparse_merge_topk(a_idx, a_val, b_idx, b_val, 2)
    assert idx.tolist() == [7, 9] and val.tolist() == [2.0, 3.0]
    idx, val = ops.sparse_merge_topk(a_idx, a_val, b_idx, b_val, 9)
    assert idx.tolist() == [2, 5, 7, 9, 11]
    assert val.tolist() == [1.0, 0.0, 2.0, 3.0, -2.0]


def test_merge_argument_checks():
    i = torch.tensor([1, 2], dtype=torch.int32)
    v = torch.tensor([1.0, 2.0])
    with pytest.raises(ValueError):
        ops.sparse_merge_topk(i, v, i, v, 0)
    with pytest.raises(TypeError):
        ops.sparse_merge_topk(i.long(), v, i, v, 1)
    with pytest.raises(TypeError):
        ops.sparse_merge_topk(i, v.double(), i, v, 1)
    with pytest.raises(TypeError):
        ops.sparse_merge_topk(i, v[:1], i, v, 1)
