"""HIP sparse_merge_topk (ops/csrc/topk_select.hip) against the torch
reference, bit for bit, and against the dense oracle of the CPU test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oktopk_amd import ops
from oktopk_amd.ops import reference as R

from test_sparse_merge import LENGTHS, dense_oracle, ks_for, make_lists


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(lists):
    a_idx, a_val, b_idx, b_val = lists
    union = torch.unique(torch.cat([a_idx, b_idx])).numel()
    dev = [x.cuda() for x in lists]
    for k in ks_for(union):
        r_idx, r_val = R.sparse_merge_topk(a_idx, a_val, b_idx, b_val, k)
        idx, val = ops.sparse_merge_topk(*dev, k)
        assert idx.dtype == torch.int32 and val.dtype == torch.float32
        assert idx.numel() == min(k, union)
        assert torch.equal(idx.cpu(), r_idx)
        assert torch.equal(_bits(val.cpu()), _bits(r_val))
    for x, d in zip(lists, dev):
        assert torch.equal(_bits(d.cpu()), _bits(x))  # inputs untouched


@pytest.mark.parametrize("overlap", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("lb", [0, 1, 64, 65, 1000])
@pytest.mark.parametrize("la", LENGTHS)
def test_merge_lengths_and_overlap(la, lb, overlap):
    _check(make_lists(la, lb, overlap, "randn", seed=la * 7 + lb))


@pytest.mark.parametrize("mode", ["randn", "quant", "cancel"])
@pytest.mark.parametrize("overlap", [0.0, 0.5, 1.0])
def test_merge_long_lists(mode, overlap):
    _check(make_lists(110_000, 110_000, overlap, mode, seed=5))


@pytest.mark.parametrize("la,lb", [(63, 65), (65, 64), (1000, 1000),
                                   (1000, 110_000)])
@pytest.mark.parametrize("mode", ["quant", "cancel"])
@pytest.mark.parametrize("overlap", [0.5, 1.0])
def test_merge_ties_and_cancellation(la, lb, mode, overlap):
    _check(make_lists(la, lb, overlap, mode, seed=13))


def test_merge_matches_dense_oracle():
    lists = make_lists(1000, 1000, 0.5, "quant", seed=21)
    dev = [x.cuda() for x in lists]
    for k in (1, 400, 1500, 5000):
        o_idx, o_val, _ = dense_oracle(*lists, k)
        idx, val = ops.sparse_merge_topk(*dev, k)
        assert torch.equal(idx.cpu(), o_idx)
        assert torch.equal(val.cpu(), o_val)
