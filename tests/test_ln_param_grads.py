"""Batched LayerNorm parameter gradients, the parts that need no GPU: the
reference restatement of torch's summation order, that CPU modules never take
the new path, and the owner's fold / materialise rule."""
import pytest
import torch

from oktopk_amd.ops.fused_linear import GradSlotOwner, LnGradSource, bind_add_slot
from oktopk_amd.ops.reference import ln_param_grads_torch_order
from oktopk_amd.ops.slot_ln import SlotLayerNorm

BF = torch.bfloat16


@pytest.mark.parametrize("N", [64, 100, 768, 1024])
@pytest.mark.parametrize("M", [128, 130, 1000, 1024])
def test_reference_order_against_fp64(M, N):
    """Every path from a term to the root of the tree has at most 17 adds
    (4 in a thread row, 2 across them, 8 over partials, 3 across those) and a
    gamma term carries 3 roundings of its own (subtract and two products), so
    |fp32 sum - exact| <= 20 * 2^-24 * sum |t| to first order; the result is
    then rounded once to bf16 (8 significant bits: 2^-8 relative)."""
    g = torch.Generator().manual_seed(1000 * M + N)
    gy = torch.randn(M, N, generator=g).to(BF)
    x = (3 * torch.randn(M, N, generator=g) + 0.5).to(BF)
    _, mean, rstd = torch.native_layer_norm(x.float(), (N,), None, None, 1e-12)
    got = ln_param_grads_torch_order(gy, x, mean, rstd)
    assert got[0].dtype == BF and got[0].shape == (N,)
    dy = gy.double()
    terms = (dy * (x.double() - mean.double().view(M, 1)) * rstd.double().view(M, 1), dy)
    for out, t in zip(got, terms):
        exact, mass = t.sum(0), t.abs().sum(0)
        fp32_err = 20 * 2.0 ** -24 * mass
        bound = fp32_err + 2.0 ** -8 * (exact.abs() + fp32_err) + 1e-40
        assert bool(((out.double() - exact).abs() <= bound).all())


def test_reference_order_is_the_written_tree():
    """Cancelling powers of two: which 1.0 an fp32 add loses tells the
    association tree apart from a row-by-row or a pairwise sum."""
    M, N, big = 130, 4, 2.0 ** 24
    gy = torch.zeros(M, N)
    # rows 0, 4, 8 share A(0): (big + 1) + -big loses the 1
    gy[0, 0], gy[4, 0], gy[8, 0] = big, 1.0, -big
    # rows 0..3 fall into A(0)..A(3): (big + -big) + (1 + 1) keeps both
    gy[0, 1], gy[1, 1], gy[2, 1], gy[3, 1] = big, 1.0, -big, 1.0
    # P(0) = big and P(1) = 1 share S(0), P(8) = -big is S(1)
    gy[0, 2], gy[16, 2], gy[128, 2] = big, 1.0, -big
    gg, gb = ln_param_grads_torch_order(gy.to(BF), torch.full((M, N), 3.0).to(BF),
                                        torch.ones(M), torch.full((M,), 0.5))
    assert gb.tolist() == [0.0, 2.0, 0.0, 0.0]
    assert gg.tolist() == [0.0, 2.0, 0.0, 0.0]       # t = (gy * (3 - 1)) * 0.5


def test_reference_rows_past_M_and_signed_zero():
    M, N = 130, 2
    gy = torch.zeros(M, N)
    gy[:, 0] = -0.0                      # every sum starts at +0.0
    gy[129, 1] = 3.0                     # the last, partial chunk counts
    gg, gb = ln_param_grads_torch_order(gy.to(BF), torch.ones(M, N).to(BF),
                                        torch.zeros(M), torch.full((M,), 2.0))
    assert gb.view(torch.int16)[0].item() == 0 and gb[1].item() == 3.0
    assert gg[1].item() == 6.0           # (3 * (1 - 0)) * 2


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_cpu_modules_never_take_the_batched_path(dtype, monkeypatch):
    monkeypatch.setenv("OKTOPK_DEFER_SMALL_GRADS", "1")
    monkeypatch.setenv("OKTOPK_BATCH_LN_GRADS", "1")
    torch.manual_seed(0)
    ln, ref = SlotLayerNorm(16).to(dtype), torch.nn.LayerNorm(16).to(dtype)
    ref.load_state_dict(ln.state_dict())
    owner = GradSlotOwner()
    for p in ln.parameters():
        p.grad = torch.zeros_like(p)
        bind_add_slot(p, p.grad, owner)
    x = torch.randn(256, 16).to(dtype)
    ln(x).float().square().sum().backward()
    ref(x).float().square().sum().backward()
    assert owner.pending == [] and not owner.written
    for p, q in zip(ln.parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad)


class FakeSource(LnGradSource):
    def __init__(self, w, b, w_dst, b_dst, gw, gb):
        z = torch.zeros(1)
        super().__init__(z, z, z, z, w, b, w_dst, b_dst)
        self.grads, self.calls = (gw, gb), 0

    def materialise(self):
        self.calls += 1
        return self.grads


def idle_owner():
    """An owner that takes entries outside a backward pass: the end-of-backward
    callback, which only a running pass accepts, counts as queued."""
    owner = GradSlotOwner()
    owner._callback_queued = True
    return owner


def test_owner_folds_onto_a_materialised_source():
    owner = idle_owner()
    w, b = (torch.nn.Parameter(torch.zeros(4, dtype=BF)) for _ in range(2))
    w_dst, b_dst = torch.zeros(4, dtype=BF), torch.zeros(4, dtype=BF)
    gw, gb = torch.full((4,), 256.0, dtype=BF), torch.full((4,), 2.0, dtype=BF)
    site = FakeSource(w, b, w_dst, b_dst, gw, gb)
    owner.defer_ln(site)
    # two entries a site, marked as adds, holding the source object
    assert [e[2] for e in owner.pending] == [False, False]
    assert owner.pending[0][0] is site and owner.pending[1][0] is site
    assert owner.pending[0][1] is w_dst and owner.pending[1][1] is b_dst
    assert owner.has_pending(w) and owner.has_pending(b) and site.calls == 0
    # the module's second use: materialise, then the bf16 fold (256 + 1 -> 256)
    owner.defer(w, torch.ones(4, dtype=BF), w_dst, False)
    assert site.calls == 1 and len(owner.pending) == 2
    assert torch.equal(owner.pending[0][0], torch.full((4,), 256.0, dtype=BF))
    assert owner.pending[1][0] is gb, "the beta entry became a plain add entry"
    owner.defer(b, torch.ones(4, dtype=BF), b_dst, False)
    assert site.calls == 1
    assert torch.equal(owner.pending[1][0], torch.full((4,), 3.0, dtype=BF))
    assert [e[2] for e in owner.pending] == [False, False]
    owner.discard()
    assert owner.pending == [] and not owner.has_pending(w)


def test_discard_drops_sources():
    owner = idle_owner()
    w, b = (torch.nn.Parameter(torch.zeros(4, dtype=BF)) for _ in range(2))
    owner.defer_ln(FakeSource(w, b, torch.zeros(4, dtype=BF), torch.zeros(4, dtype=BF),
                              None, None))
    assert len(owner.pending) == 2
    owner.discard()
    assert owner.pending == [] and not owner.has_pending(w) and not owner.has_pending(b)
    assert not owner._callback_queued
