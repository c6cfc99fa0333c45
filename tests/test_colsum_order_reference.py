"""reference.colsum_torch_order: the CPU emulation of the order in which
torch's GPU reduction adds a column (documentation of what the native
colsum_bf16_into_exact reproduces)."""
import pytest
import torch

from oktopk_amd.ops.reference import colsum_torch_order


def _cancelling(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    q = R // 4
    big = (64 * torch.randn(q, C, generator=g)).bfloat16()
    small = (1e-3 * torch.randn(R - 2 * q, C, generator=g)).bfloat16()
    x = torch.cat([big, -big, small], 0)
    return x.gather(0, torch.rand(R, C, generator=g).argsort(0))


def _sequential(x):
    s = torch.zeros(x.shape[1], dtype=torch.float32)
    for r in range(x.shape[0]):
        s = s + x[r].float()
    return s


@pytest.mark.parametrize("R,C", [(1, 5), (7, 3), (300, 64), (1024, 48)])
def test_degenerate_parameters_are_a_sequential_sum(R, C):
    x = _cancelling(R, C, R + C)
    got = colsum_torch_order(x, bh=1, ctas=1, vt0=1)
    assert torch.equal(got.view(torch.int32), _sequential(x).view(torch.int32))


@pytest.mark.parametrize("R,C,bh,ctas", [(1024, 768, 2, 32), (1024, 96, 4, 1),
                                         (300, 64, 2, 1), (1027, 40, 2, 32),
                                         (4096, 16, 2, 128)])
def test_within_fp32_bound_of_fp64_sum(R, C, bh, ctas):
    x = _cancelling(R, C, 3 * R + C)
    got = colsum_torch_order(x, bh=bh, ctas=ctas, vt0=4).double()
    ref = x.double().sum(0)
    bound = R * 2.0 ** -24 * x.double().abs().sum(0)
    assert ((got - ref).abs() <= bound).all()


def test_order_is_visible_on_cancelling_columns():
    """The data the GPU test uses separates orders: torch's workload order
    vs a sequential sum, and ctas = 32 vs ctas = 16, after the bf16
    rounding."""
    x = _cancelling(1024, 768, 9)
    a = colsum_torch_order(x, 2, 32, 4).bfloat16()
    seq = _sequential(x).bfloat16()
    b = colsum_torch_order(x, 2, 16, 4).bfloat16()
    assert (a.view(torch.int16) != seq.view(torch.int16)).sum() > 0
    assert (a.view(torch.int16) != b.view(torch.int16)).sum() > 0


def test_accumulator_assignment():
    # rows 0..9 of one lane (bh = ctas = 1): A0 = r0+r4+r8, A1 = r1+r5+r9,
    # A2 = r2+r6, A3 = r3+r7, result ((A0+A1)+A2)+A3
    x = _cancelling(10, 6, 2).float()
    a = [x[0] + x[4] + x[8], x[1] + x[5] + x[9], x[2] + x[6], x[3] + x[7]]
    want = ((a[0] + a[1]) + a[2]) + a[3]
    got = colsum_torch_order(x, 1, 1, 4)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
