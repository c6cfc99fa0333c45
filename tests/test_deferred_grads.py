"""Deferred small gradient writes, the parts that need no GPU: the reference
add rule, that nothing but a bound bf16 GPU module ever defers, and that
zero_grad() forgets what a failed backward left in the list."""
import types

import pytest
import torch

from oktopk_amd.ops.fused_linear import (ColsumLinear, GradSlotOwner,
                                         bind_add_slot, bind_grad_slot)
from oktopk_amd.ops.reference import slot_add_bf16
from oktopk_amd.ops.slot_ln import SlotLayerNorm

BF = torch.bfloat16


def bits(t):
    return t.contiguous().view(torch.int16)


def test_reference_add_rule():
    inf, nan, sub = float("inf"), float("nan"), 2e-40
    a = torch.tensor([-0.0, -0.0, 0.0, 1.0, inf, inf, sub, 1.0, 256.0, 256.0]).to(BF)
    b = torch.tensor([0.0, -0.0, -0.0, -1.0, 1.0, -inf, sub, nan, 1.0, 3.0]).to(BF)
    got = slot_add_bf16(a, b)
    assert got.dtype == BF
    # signed zeros: only -0 + -0 keeps the sign; x - x is +0
    assert bits(got)[:4].tolist() == [0, -32768, 0, 0]
    assert got[4].item() == inf and got[5].isnan() and got[7].isnan()
    # subnormals are added, not flushed: 2 * sub, exact
    assert got[6].item() == (a[6].float() * 2).item() != 0.0
    # one rounding to nearest even at 8 bits: 257 -> 256, 259 -> 260
    assert got[8].item() == 256.0 and got[9].item() == 260.0
    # the in-place bf16 add it stands for
    fin = torch.randn(4096).to(BF), (0.01 * torch.randn(4096)).to(BF)
    assert torch.equal(bits(slot_add_bf16(*fin)), bits(fin[0].clone().add_(fin[1])))


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("bound", [False, True])
def test_cpu_modules_never_defer(dtype, bound, monkeypatch):
    monkeypatch.setenv("OKTOPK_DEFER_SMALL_GRADS", "1")
    torch.manual_seed(0)
    lin, ln = ColsumLinear(16, 16).to(dtype), SlotLayerNorm(16).to(dtype)
    ref_lin, ref_ln = torch.nn.Linear(16, 16).to(dtype), torch.nn.LayerNorm(16).to(dtype)
    ref_lin.load_state_dict(lin.state_dict())
    ref_ln.load_state_dict(ln.state_dict())
    owner = GradSlotOwner()
    if bound:
        for p in lin.parameters():
            p.grad = torch.zeros_like(p)
            bind_grad_slot(p, p.grad, owner)
        for p in ln.parameters():
            p.grad = torch.zeros_like(p)
            bind_add_slot(p, p.grad, owner)
    x = torch.randn(8, 16).to(dtype)
    ln(lin(x)).float().square().sum().backward()
    ref_ln(ref_lin(x)).float().square().sum().backward()
    assert owner.pending == [] and not owner.written
    for p, q in zip(list(lin.parameters()) + list(ln.parameters()),
                    list(ref_lin.parameters()) + list(ref_ln.parameters())):
        assert torch.equal(p.grad, q.grad)


def test_zero_grad_clears_what_a_failed_backward_left(monkeypatch):
    from oktopk_amd.optimizer import FlatBertAdam

    # defer() on CPU tensors: only the stream lookup needs a device
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    owner = GradSlotOwner()
    p = torch.nn.Parameter(torch.zeros(4, dtype=BF))
    slot = torch.zeros(4, dtype=BF)

    class Defers(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            owner.defer(p, torch.ones(4, dtype=BF), slot, False)
            return g

    class Raises(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError("backward failed")

    x = torch.zeros(4, requires_grad=True)
    with pytest.raises(RuntimeError, match="backward failed"):
        Raises.apply(Defers.apply(x)).sum().backward()    # never reached ...
    assert owner.pending == []
    with pytest.raises(RuntimeError, match="backward failed"):
        Defers.apply(Raises.apply(x)).sum().backward()    # ... deferred, then raised
    assert len(owner.pending) == 1 and owner.has_pending(p)

    flat = torch.ones(8, dtype=BF)
    opt = types.SimpleNamespace(_dg_owner=owner, _zero_ranges=None,
                                flat_grad_model=flat, params=[], slots=[],
                                _settle_direct_grad=lambda: None)
    FlatBertAdam.zero_grad(opt)
    assert owner.pending == [] and not owner.has_pending(p)
    assert not owner._callback_queued, "the next backward registers its own flush"
    assert float(flat.abs().max()) == 0.0
