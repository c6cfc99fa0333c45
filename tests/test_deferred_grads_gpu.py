"""small_grads_batched (ops/csrc/direct_grad.hip) and the deferral built on
it (GradSlotOwner in ops/fused_linear.py, SlotLayerNorm).

The batched launch must leave the raw 16-bit patterns that the launches it
replaces leave: colsum_bf16_into_exact per bias and `slot.add_(g)` per
LayerNorm gradient.  The node-level tests compare whole flat gradient buffers
with OKTOPK_DEFER_SMALL_GRADS on and off.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# (R, C, lead): lead elements into the allocation.  With 256 CUs torch's
# configuration (bh, ctas) and the load width differ from entry to entry:
#   64x8 rows not split, 16-B loads      128x96 bh 8, 16-B loads
#   256x770, 130x1026 bh 4, 4-B loads, odd strips
#   300x250 at lead 1: 2-B loads         1024x768 bh 2, ctas 32 (the bench shape)
COLSUM_SHAPES = [(64, 8, 0), (128, 96, 0), (256, 770, 0), (130, 1026, 0),
                 (300, 250, 1), (1024, 768, 0)]


def hip():
    from oktopk_amd import _hip_ops
    return _hip_ops


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    """Raw patterns equal; where both hold a NaN the payload is not compared."""
    nan = a.float().isnan() & b.float().isnan()
    return bool(((bits(a) == bits(b)) | nan).all())


def source(R, C, lead, seed):
    """bf16 [R, C] with cancelling columns (a summation order shows in the
    bits), starting `lead` elements into its allocation."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = R // 4
    big = (64 * torch.randn(q, C, device="cuda", generator=g)).to(BF)
    small = (1e-3 * torch.randn(R - 2 * q, C, device="cuda", generator=g)).to(BF)
    x = torch.cat([big, -big, small], 0)
    x = x.gather(0, torch.rand(R, C, device="cuda", generator=g).argsort(0))
    store = torch.empty(R * C + 8, dtype=BF, device="cuda")
    view = store[lead:lead + R * C].view(R, C)
    view.copy_(x)
    return view


def special_adds(n, seed):
    """(slot, g) of n elements: random values, with -0.0 + +0.0, -0.0 + -0.0,
    infinities of both and opposite signs, subnormals and a NaN in front."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    slot = torch.randn(n, device="cuda", generator=gen).to(BF)
    g = (torch.randn(n, device="cuda", generator=gen) * 0.01).to(BF)
    sub = 2e-40
    a = [-0.0, -0.0, float("inf"), float("inf"), float("-inf"), sub, -sub, sub, float("nan"), 1.0]
    b = [0.0, -0.0, 1.0, float("-inf"), float("-inf"), sub, sub, 3e-39, 1.0, float("nan")]
    k = min(n, len(a))
    slot[:k] = torch.tensor(a[:k], device="cuda").to(BF)
    g[:k] = torch.tensor(b[:k], device="cuda").to(BF)
    return slot, g


class Flat:
    """One flat bf16 buffer; slots are handed out at odd element offsets with
    sentinel elements between them."""
    SENTINEL = 7.0

    def __init__(self, numel):
        self.buf = torch.full((numel,), self.SENTINEL, dtype=BF, device="cuda")
        self.used = 1
        self.slots = []

    def slot(self, n):
        off = self.used + (1 - self.used % 2)      # odd offset
        assert off + n + 1 <= self.buf.numel()
        self.slots.append((off, n))
        self.used = off + n + 1
        return self.buf[off:off + n]

    def sentinels_intact(self):
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for off, n in self.slots:
            keep[off:off + n] = False
        return bool((self.buf[keep] == self.SENTINEL).all())


def run_both(specs):
    """specs: ("colsum", gy) or ("add", slot_init, g).  Runs them through the
    single launches and through one batched call into two identically laid
    out flat buffers.  Returns (launches, want Flat, got Flat)."""
    total = sum((s[1].shape[-1] + 3) for s in specs) + 8
    want, got = Flat(total), Flat(total)
    entries = []
    for s in specs:
        n = s[1].shape[-1]
        w, g = want.slot(n), got.slot(n)
        if s[0] == "colsum":
            assert hip().colsum_exact_deferrable(s[1])
            assert hip().colsum_bf16_into_exact(s[1], w, False)
            entries.append((s[1], g, True))
        else:
            w.copy_(s[1])
            g.copy_(s[1])
            w.add_(s[2])
            entries.append((s[2], g, False))
    launches = hip().small_grads_batched(entries)
    torch.cuda.synchronize()
    return launches, want, got


def check(specs, launches_expected):
    launches, want, got = run_both(specs)
    assert launches == launches_expected
    assert got.sentinels_intact() and want.sentinels_intact()
    for (off, n), s in zip(got.slots, specs):
        assert same_bits(got.buf[off:off + n], want.buf[off:off + n]), \
            f"{s[0]} entry of {n} elements at offset {off}"


@pytest.fixture(scope="module")
def sources():
    return [source(R, C, lead, 100 + i) for i, (R, C, lead) in enumerate(COLSUM_SHAPES)]


def test_mixed_configurations_in_one_launch(sources):
    specs = []
    for i, gy in enumerate(sources):
        specs.append(("colsum", gy))
        specs.append(("add",) + special_adds(gy.shape[1], 7 + i))
    check(specs, 1)
    # the yardstick of the single op itself: torch's reduction
    _, want, _ = run_both(specs[::2])
    for (off, n), gy in zip(want.slots, sources):
        ref = torch.empty(n, dtype=BF, device="cuda")
        torch.sum(gy, 0, out=ref)
        assert torch.equal(bits(want.buf[off:off + n]), bits(ref))


def test_add_special_values_and_reference_rule():
    from oktopk_amd.ops.reference import slot_add_bf16

    slot, g = special_adds(1500, 3)       # three blocks, a partial last one
    assert slot[0].item() == 0 and g[5].float().abs().item() < 1.2e-38
    check([("add", slot, g)], 1)
    got = slot.clone()
    hip().small_grads_batched([(g, got, False)])
    assert same_bits(got, slot_add_bf16(slot, g))
    assert bits(got)[0].item() == 0, "-0.0 + +0.0 is +0.0"
    assert bits(got)[1].item() == -32768, "-0.0 + -0.0 is -0.0"
    assert got[3].float().isnan() and got[8].float().isnan() and got[9].float().isnan()
    # onto a zeroed slot: the value itself, -0.0 excepted
    zero = torch.zeros_like(g)
    hip().small_grads_batched([(g, zero, False)])
    assert same_bits(zero, g + torch.zeros_like(g))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_capacity_boundary(delta):
    cap = hip().GRAD_BATCH_CAPACITY
    n = cap + delta
    small = source(64, 8, 0, 5)
    specs = []
    for i in range(n):
        if i % 3 == 0:
            specs.append(("colsum", small))
        else:
            specs.append(("add",) + special_adds(5 + i % 7, i))
    # the last entry, alone in a second launch at cap + 1, needs LDS itself
    specs[-1] = ("colsum", source(128, 96, 0, 6))
    check(specs, 1 if n <= cap else 2)


def test_empty_list_launches_nothing():
    assert hip().small_grads_batched([]) == 0
    empty = torch.empty(0, dtype=BF, device="cuda")
    assert hip().small_grads_batched([(empty, empty, False)]) == 0


def test_unsupported_entry_is_refused_before_any_launch():
    one_row = torch.ones(1, 64, dtype=BF, device="cuda")
    assert not hip().colsum_exact_deferrable(one_row)
    assert not hip().colsum_exact_deferrable(torch.ones(64, 1, dtype=BF, device="cuda"))
    assert not hip().colsum_exact_deferrable(torch.ones(64, 16, dtype=BF, device="cuda").t())
    slot, g = special_adds(64, 1)
    before = slot.clone()
    dst = torch.full((64,), 7.0, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError):
        hip().small_grads_batched([(g, slot, False), (one_row, dst, True)])
    torch.cuda.synchronize()
    assert same_bits(slot, before) and bool((dst == 7.0).all())


# -- node level ---------------------------------------------------------------

H, ROWS = 128, 64


class Net(torch.nn.Module):
    def __init__(self, twice):
        super().__init__()
        from oktopk_amd.ops.fused_linear import ColsumLinear
        from oktopk_amd.ops.slot_ln import SlotLayerNorm

        self.twice = twice
        self.l1, self.n1 = ColsumLinear(H, H), SlotLayerNorm(H, eps=1e-12)
        self.l2, self.n2 = ColsumLinear(H, H), SlotLayerNorm(H, eps=1e-12)

    def forward(self, x):
        h = self.n1(torch.nn.functional.gelu(self.l1(x)))
        if self.twice:
            h = self.n1(self.l1(h))
        return self.n2(self.l2(h) + h)


class Arm:
    """The model bound to a flat gradient buffer the way FlatBertAdam binds
    it: Linear parameters own their slots, LayerNorm slots are zeroed and,
    with the switch on, bound as add slots."""

    def __init__(self, monkeypatch, defer, twice=False):
        from oktopk_amd.ops.fused_linear import (GradSlotOwner, bind_add_slot,
                                                 bind_grad_slot)

        monkeypatch.setenv("OKTOPK_DEFER_SMALL_GRADS", "1" if defer else "0")
        monkeypatch.delenv("OKTOPK_COLSUM_BIAS", raising=False)
        torch.manual_seed(11)
        self.model = Net(twice).to(BF).cuda()
        with torch.no_grad():
            for m in (self.model.n1, self.model.n2):
                m.weight.add_(0.1 * torch.randn_like(m.weight))
        params = list(self.model.parameters())
        self.flat = Flat(sum(p.numel() + 3 for p in params) + 8)
        self.owner = GradSlotOwner()
        self.zeroed = []
        for p in params:
            slot = self.flat.slot(p.numel()).view_as(p)
            p.grad = slot
            if p.dim() == 2 or p is self.model.l1.bias or p is self.model.l2.bias:
                bind_grad_slot(p, slot, self.owner)
            else:
                self.zeroed.append(slot)
                if defer:
                    bind_add_slot(p, slot, self.owner)

    def zero_grad(self):
        self.owner.discard()
        self.owner.written.clear()
        for s in self.zeroed:
            s.zero_()

    def backward(self, x):
        y = self.model(x)
        (y.float() * self.weights).sum().backward()

    weights = None


def inputs(n):
    g = torch.Generator(device="cuda").manual_seed(23)
    xs = [torch.randn(ROWS, H, device="cuda", generator=g).to(BF) for _ in range(n)]
    w = torch.randn(ROWS, H, device="cuda", generator=g)
    return xs, w


def run_arm(monkeypatch, defer, twice=False, per_zero=1):
    """Flat buffers after each zero_grad() group of backward passes."""
    arm = Arm(monkeypatch, defer, twice)
    xs, arm.weights = inputs(3 * per_zero)
    out = []
    for i in range(3):
        arm.zero_grad()
        for x in xs[i * per_zero:(i + 1) * per_zero]:
            arm.backward(x)
            assert arm.owner.pending == [], "flushed when backward() returns"
        torch.cuda.synchronize()
        assert arm.flat.sentinels_intact()
        out.append(arm.flat.buf.clone())
    return arm, out


@pytest.mark.parametrize("twice,per_zero", [(False, 1), (False, 2), (True, 1)],
                         ids=["plain", "accumulate", "module_twice"])
def test_flat_buffer_equal_on_and_off(monkeypatch, twice, per_zero):
    _, off = run_arm(monkeypatch, False, twice, per_zero)
    arm, on = run_arm(monkeypatch, True, twice, per_zero)
    assert len(arm.owner.written) == 4
    for a, b in zip(on, off):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(bits(on[0]), bits(on[1])), "inputs differ per pass"


def test_deferral_happens_and_batches(monkeypatch):
    """With the switch on the nodes launch nothing themselves: all 2 biases
    and 4 LayerNorm gradients are in the list when the backward ends."""
    arm = Arm(monkeypatch, True)
    xs, arm.weights = inputs(1)
    seen = []
    flush = arm.owner.flush

    def spy():
        seen.append([e[2] for e in arm.owner.pending])
        flush()
    arm.owner.flush = spy
    arm.zero_grad()
    arm.backward(xs[0])
    assert sorted(seen[0]) == [False] * 4 + [True] * 2
    assert arm.owner.pending == []


def test_references_dropped_after_flush(monkeypatch):
    deltas = []
    for defer in (False, True):
        arm = Arm(monkeypatch, defer)
        xs, arm.weights = inputs(2)
        arm.zero_grad()
        arm.backward(xs[0])                # first use: caches, workspaces
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        arm.zero_grad()
        arm.backward(xs[1])
        torch.cuda.synchronize()
        deltas.append(torch.cuda.memory_allocated() - before)
    assert deltas[0] == deltas[1] == 0


def test_captured_graph_replays(monkeypatch):
    xs, w = inputs(3)
    ref_arm = Arm(monkeypatch, False)
    ref_arm.weights = w
    want = []
    for x in xs:
        ref_arm.zero_grad()
        ref_arm.backward(x)
        want.append(ref_arm.flat.buf.clone())

    arm = Arm(monkeypatch, True)
    arm.weights = w
    static_x = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            arm.zero_grad()
            arm.backward(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        arm.zero_grad()
        arm.backward(static_x)
    assert arm.owner.pending == []
    for x, ref in zip(xs, want):
        arm.flat.buf[1:].fill_(3.0)        # replay must rewrite every slot
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for off, n in arm.flat.slots:
            assert torch.equal(bits(arm.flat.buf[off:off + n]),
                               bits(ref[off:off + n]))
