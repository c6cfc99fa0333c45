"""Exact top-k selection, reference backend (CPU): ops.topk_select and
ops.topk_select_ef against an independent oracle — a stable descending sort
of |x|, the first k, indices re-sorted."""
import pytest
import torch

from oktopk_amd import ops


def oracle(x: torch.Tensor, k: int):
    k = min(k, x.numel())
    order = torch.sort(x.abs(), descending=True, stable=True).indices[:k]
    idx = torch.sort(order).values
    return idx.to(torch.int32), x[idx], float(x.abs()[order[-1]])


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int32)


def _inputs():
    g = torch.Generator().manual_seed(11)
    n = 5000
    randn = torch.randn(n, generator=g)
    return {
        "randn": randn,
        "zeros": torch.zeros(n),
        "const": torch.full((n,), -0.75),
        "quant": torch.round(torch.randn(n, generator=g) * 4) / 4,
        "one": torch.tensor([-3.5]),
    }


INPUTS = _inputs()


@pytest.mark.parametrize("name", ["randn", "zeros", "const", "quant"])
@pytest.mark.parametrize("k", [1, 5, 250, 4999, 5000, 7000])
def test_topk_select_matches_sort_oracle(name, k):
    x = INPUTS[name]
    before = x.clone()
    idx, val, tau = ops.topk_select(x, k)
    o_idx, o_val, o_tau = oracle(x, k)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32
    assert idx.numel() == min(k, x.numel())
    assert torch.equal(idx, o_idx)
    assert torch.equal(bits(val), bits(o_val))
    assert tau == o_tau
    assert torch.equal(bits(x), bits(before))  # plain variant writes nothing


@pytest.mark.parametrize("k", [1, 2])
def test_topk_select_single_element(k):
    idx, val, tau = ops.topk_select(INPUTS["one"], k)
    assert idx.tolist() == [0] and val.tolist() == [-3.5] and tau == 3.5


def test_tie_class_filled_from_lowest_index():
    x = torch.tensor([1.0, -2.0, 2.0, 0.5, -2.0, 3.0, 2.0])
    idx, val, tau = ops.topk_select(x, 3)
    assert idx.tolist() == [1, 2, 5]  # 3.0, then the first two of four 2.0s
    assert val.tolist() == [-2.0, 2.0, 3.0]
    assert tau == 2.0


def test_signed_zero_magnitudes_tie():
    x = torch.tensor([0.0, -0.0, 0.0, -0.0])
    idx, val, tau = ops.topk_select(x, 2)
    assert idx.tolist() == [0, 1]
    assert torch.equal(bits(val), bits(x[:2]))
    assert tau == 0.0


@pytest.mark.parametrize("name", ["randn", "quant", "zeros", "const"])
@pytest.mark.parametrize("with_grad", [False, True])
@pytest.mark.parametrize("k", [1, 37, 5000, 9999])
def test_topk_select_ef_residual_postcondition(name, with_grad, k):
    g = torch.Generator().manual_seed(3)
    t = INPUTS[name].clone()
    n = t.numel()
    residual = torch.round(torch.randn(n, generator=g) * 2) / 2 \
        if name == "quant" else torch.randn(n, generator=g) * 0.5
    if name in ("zeros", "const"):
        residual = torch.zeros(n)
    grad = t.to(torch.bfloat16) if with_grad else None
    restored = (grad.float() if with_grad else t) + residual
    t_before = t.clone()
    r = residual.clone()
    idx, val, tau = ops.topk_select_ef(t, r, grad, k)
    o_idx, o_val, o_tau = oracle(restored, k)
    assert torch.equal(idx, o_idx)
    assert torch.equal(bits(val), bits(o_val))
    assert tau == o_tau
    assert torch.equal(bits(t), bits(t_before))  # t is not written
    expect = restored.clone()
    expect[o_idx.long()] = 0.0
    assert torch.equal(bits(r), bits(expect))  # +0.0 at the selection
    # what was sent plus what was kept is the restored gradient
    dense = torch.zeros(n)
    dense[idx.long()] = val
    assert torch.equal(dense + r, restored)


def test_argument_checks():
    t = torch.randn(16)
    r = torch.zeros(16)
    with pytest.raises(ValueError):
        ops.topk_select(t, 0)
    with pytest.raises(ValueError):
        ops.topk_select_ef(t, r, None, -1)
    with pytest.raises(TypeError):
        ops.topk_select(t.double(), 3)
    with pytest.raises(TypeError):
        ops.topk_select_ef(t, r.double(), None, 3)
    with pytest.raises(TypeError):
        ops.topk_select_ef(t, torch.zeros(15), None, 3)
    with pytest.raises(TypeError):
        ops.topk_select_ef(t, r, t.half(), 3)  # grad must be bf16
    with pytest.raises(TypeError):
        ops.topk_select_ef(t, r, t.to(torch.bfloat16)[:8], 3)
    with pytest.raises(TypeError):
        ops.topk_select(torch.empty(0), 1)
