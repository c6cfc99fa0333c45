"""ln_param_grads_batched (ops/csrc/ln_param_grads.hip) and the deferral built
on it, against what they stand in for: torch's
native_layer_norm_backward(..., [False, True, True]) followed by the bf16
`slot += g`.  Raw 16-bit patterns are compared, NaN included.  A torch whose
gamma / beta reduction sums in another order shows up here as a bit mismatch;
OKTOPK_BATCH_LN_GRADS=0 is the way back.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 1e-12
ROWS = [128, 130, 1000, 1024]
COLS = [64, 100, 768, 1024]
SENTINEL = 7.0


def hip():
    from oktopk_amd import _hip_ops
    return _hip_ops


def bits(t):
    return t.contiguous().view(torch.int16)


class Site:
    """One LayerNorm site: gy and x with cancelling rows (a summation order
    shows in the bits), the row statistics native_layer_norm leaves for x."""

    def __init__(self, M, N, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        q = M // 4
        big = 64 * torch.randn(q, N, device="cuda", generator=g)
        gy = torch.cat([big, -big, 1e-3 * torch.randn(M - 2 * q, N, device="cuda",
                                                      generator=g)], 0)
        self.gy = gy.gather(0, torch.rand(M, N, device="cuda", generator=g).argsort(0)).to(BF)
        self.x = (3 * torch.randn(M, N, device="cuda", generator=g) + 0.5).to(BF)
        self.w = torch.randn(N, device="cuda", generator=g).to(BF)
        self.b = torch.randn(N, device="cuda", generator=g).to(BF)
        self.slot_init = torch.randn(2, N, device="cuda", generator=g).to(BF)
        self.restat()

    def restat(self):
        N = self.x.shape[-1]
        _, self.mean, self.rstd = torch.native_layer_norm(self.x, (N,), self.w, self.b, EPS)

    def torch_grads(self):
        N = self.x.shape[-1]
        return torch.ops.aten.native_layer_norm_backward(
            self.gy, self.x, [N], self.mean, self.rstd, self.w, self.b,
            [False, True, True])[1:]


def flat_slots(sites):
    """A flat bf16 buffer of sentinels with a (gamma, beta) slot pair per
    site at odd element offsets, holding the sites' initial slot values."""
    buf = torch.full((sum(2 * s.x.shape[-1] + 4 for s in sites) + 2,), SENTINEL,
                     dtype=BF, device="cuda")
    slots, keep, off = [], torch.ones_like(buf, dtype=torch.bool), 1
    for s in sites:
        N = s.x.shape[-1]
        pair = []
        for k in range(2):
            off += 1 - off % 2
            buf[off:off + N] = s.slot_init[k]
            keep[off:off + N] = False
            pair.append(buf[off:off + N])
            off += N + 1
        slots.append(pair)
    return buf, slots, keep


def check(sites):
    """Both ways into identically laid out buffers; returns the launches."""
    want, wslots, keep = flat_slots(sites)
    got, gslots, _ = flat_slots(sites)
    for s, (wg, wb) in zip(sites, wslots):
        gw, gb = s.torch_grads()
        wg.add_(gw)
        wb.add_(gb)
    entries = []
    for s, (gg, gb) in zip(sites, gslots):
        assert hip().ln_param_grads_deferrable(s.gy, s.x, s.mean, s.rstd)
        entries.append((s.gy, s.x, s.mean, s.rstd, gg, gb))
    launches = hip().ln_param_grads_batched(entries)
    torch.cuda.synchronize()
    assert bool((got[keep] == SENTINEL).all()), "a sentinel was overwritten"
    for i, ((wg, wb), (gg, gb)) in enumerate(zip(wslots, gslots)):
        shape = tuple(sites[i].x.shape)
        assert torch.equal(bits(gg), bits(wg)), f"gamma gradient of entry {i} {shape}"
        assert torch.equal(bits(gb), bits(wb)), f"beta gradient of entry {i} {shape}"
    assert not torch.equal(bits(got), bits(flat_slots(sites)[0])), "nothing was added"
    return launches


@pytest.fixture(scope="module")
def grid():
    return {(M, N): Site(M, N, 1000 * i + j)
            for i, M in enumerate(ROWS) for j, N in enumerate(COLS)}


@pytest.mark.parametrize("N", COLS)
@pytest.mark.parametrize("M", ROWS)
def test_one_entry_matches_torch(grid, M, N):
    assert check([grid[M, N]]) == 1


def test_flagship_shape_is_supported(grid):
    s = Site(1024, 768, 5)
    x3 = s.x.view(8, 128, 768)
    assert hip().ln_param_grads_deferrable(s.gy.view(8, 128, 768), x3,
                                           s.mean.view(8, 128, 1), s.rstd.view(8, 128, 1))
    assert check([s]) == 1


def test_entries_of_different_shapes_in_one_launch(grid):
    assert check(list(grid.values())) == 1


def test_more_entries_than_one_table_holds():
    # N = 64, 63, 62: 8-, 2- and 4-byte loads
    sites = [Site(128 + i % 4, 64 - i % 3, 50 + i) for i in range(100)]
    assert check(sites) > 1


def test_empty_list_launches_nothing():
    assert hip().ln_param_grads_batched([]) == 0


def test_special_values():
    s = Site(130, 100, 9)
    s.gy[5] = -0.0            # a row of -0.0
    s.gy[:, 3] = -0.0         # a column of it: both sums are +0.0, not -0.0
    s.gy[7, 11] = float("inf")
    s.gy[129, 13] = float("nan")
    s.x[20, 17] = float("inf")
    s.restat()                # row 20: NaN statistics, so a NaN in every gamma sum
    sub = 2e-40
    s.slot_init[:, :3] = torch.tensor([sub, -sub, 3e-39], device="cuda").to(BF)
    s.slot_init[:, 3] = -0.0
    assert 0 < s.slot_init[0, 0].float().item() < 1.2e-38
    check([s])
    t = Site(128, 64, 10)     # finite statistics: the specials reach single columns
    t.gy[5] = -0.0
    t.gy[:, 3] = -0.0
    t.gy[7, 11] = float("inf")
    t.gy[100, 13] = float("nan")
    t.slot_init[:, :3] = torch.tensor([sub, -sub, 3e-39], device="cuda").to(BF)
    t.slot_init[:, 3] = -0.0
    want, wslots, _ = flat_slots([t])
    check([t])
    gw, gb = t.torch_grads()
    assert bits(gb)[3].item() == 0 and gb[11].item() == float("inf") and gb[13].isnan()
    assert bits(wslots[0][1].add_(gb))[3].item() == 0, "-0.0 + +0.0 is +0.0"


def test_unsupported_sites_are_refused_before_any_launch(grid):
    ok = grid[128, 64]
    for M in (32, 127):
        s = Site(M, 64, M)
        assert not hip().ln_param_grads_deferrable(s.gy, s.x, s.mean, s.rstd)
    assert not hip().ln_param_grads_deferrable(ok.gy.float(), ok.x.float(), ok.mean, ok.rstd)
    tr = Site(64, 128, 3)
    assert tr.gy.t().shape == ok.gy.shape
    assert not hip().ln_param_grads_deferrable(tr.gy.t(), ok.x, ok.mean, ok.rstd)
    assert not hip().ln_param_grads_deferrable(ok.gy.cpu(), ok.x.cpu(), ok.mean.cpu(),
                                               ok.rstd.cpu())
    small = Site(127, 64, 4)
    buf, ((g0, b0), (g1, b1)), _ = flat_slots([ok, small])
    before = buf.clone()
    for bad in ((small.gy, small.x, small.mean, small.rstd, g1, b1),
                (tr.gy.t(), ok.x, ok.mean, ok.rstd, g1, b1),
                (ok.gy.float(), ok.x.float(), ok.mean, ok.rstd, g1, b1)):
        with pytest.raises(RuntimeError):
            hip().ln_param_grads_batched(
                [(ok.gy, ok.x, ok.mean, ok.rstd, g0, b0), bad])
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(before))


def test_reference_order_matches_kernel(grid):
    from oktopk_amd.ops.reference import ln_param_grads_torch_order, slot_add_bf16

    s = grid[130, 100]
    gw, gb = s.torch_grads()
    rg, rb = ln_param_grads_torch_order(s.gy.cpu(), s.x.cpu(), s.mean.cpu(), s.rstd.cpu())
    assert torch.equal(bits(rg), bits(gw.cpu())) and torch.equal(bits(rb), bits(gb.cpu()))
    slot = s.slot_init.clone()
    hip().ln_param_grads_batched([(s.gy, s.x, s.mean, s.rstd, slot[0], slot[1])])
    assert torch.equal(bits(slot[0].cpu()), bits(slot_add_bf16(s.slot_init[0].cpu(), rg)))
    assert torch.equal(bits(slot[1].cpu()), bits(slot_add_bf16(s.slot_init[1].cpu(), rb)))


# -- model level --------------------------------------------------------------

SEQ, BS, HID = 64, 2, 768      # 128 rows: the smallest the new path takes


class TinyBert(torch.nn.Module):
    """An embedding-style SlotLayerNorm, then two BertLayers (four residual
    LayerNorm sites); `twice` runs the first layer a second time."""

    def __init__(self, twice, p=0.1):
        super().__init__()
        from oktopk_amd.models.bert import BertConfig, BertLayer
        from oktopk_amd.ops.slot_ln import SlotLayerNorm

        cfg = BertConfig(hidden_size=HID, num_attention_heads=12,
                         intermediate_size=4 * HID, hidden_dropout_prob=p,
                         attention_probs_dropout_prob=p)
        self.twice = twice
        self.ln = SlotLayerNorm(HID, eps=cfg.layer_norm_eps)
        self.layer = torch.nn.ModuleList(BertLayer(cfg) for _ in range(2))

    def forward(self, x):
        x = self.layer[0](self.ln(x), None)
        if self.twice:
            x = self.layer[0](x, None)
        return self.layer[1](x, None)


class Arm:
    """The model bound the way FlatBertAdam binds it: parameters aliased into
    one bf16 buffer (the LayerNorm ones 4 bytes off an 8-byte boundary, as
    behind the flagship's decoder bias), .grad into a flat gradient buffer,
    Linear parameters owning their slots, LayerNorm slots zeroed and bound as
    add slots."""

    def __init__(self, monkeypatch, batched, twice=False, p=0.1):
        from oktopk_amd import _hip_ops
        from oktopk_amd.ops.fused_linear import (GradSlotOwner, bind_add_slot,
                                                 bind_grad_slot)
        from oktopk_amd.ops.slot_ln import SlotLayerNorm

        monkeypatch.setenv("OKTOPK_BATCH_LN_GRADS", "1" if batched else "0")
        monkeypatch.setenv("OKTOPK_DEFER_SMALL_GRADS", "1")
        monkeypatch.setenv("OKTOPK_FUSED_RESIDUAL_LN", "1")
        for k in ("OKTOPK_DIRECT_LN", "OKTOPK_COLSUM_BIAS"):
            monkeypatch.delenv(k, raising=False)
        torch.manual_seed(11)
        self.model = TinyBert(twice, p).to(BF).cuda().train()
        ln_params = {id(q) for m in self.model.modules()
                     if isinstance(m, SlotLayerNorm) for q in m.parameters()}
        params = list(self.model.parameters())
        total = sum(q.numel() + 16 for q in params)
        self.flat_param = torch.zeros(total, dtype=BF, device="cuda")
        self.flat = torch.zeros(total, dtype=BF, device="cuda")
        self.owner = GradSlotOwner()
        self.zeroed = []
        off = 0
        with torch.no_grad():
            for q in params:
                off = (off + 7) // 8 * 8 + (2 if id(q) in ln_params else 0)
                n = q.numel()
                dst = self.flat_param[off:off + n].view_as(q)
                dst.copy_(q)
                if id(q) in ln_params:
                    dst.add_(0.1 * torch.randn_like(dst))
                q.data = dst
                slot = self.flat[off:off + n].view_as(q)
                q.grad = slot
                if id(q) in ln_params:
                    self.zeroed.append(slot)
                    bind_add_slot(q, slot, self.owner)
                else:
                    bind_grad_slot(q, slot, self.owner)
                off += n
        self.sites = []             # entries per call of the new binding
        # an earlier arm of the same test may have left its spy in place
        real = getattr(_hip_ops.ln_param_grads_batched, "real",
                       _hip_ops.ln_param_grads_batched)

        def spy(entries):
            self.sites.append(len(entries))
            return real(entries)

        spy.real = real
        monkeypatch.setattr(_hip_ops, "ln_param_grads_batched", spy)

    def zero_grad(self):
        self.owner.discard()
        self.owner.written.clear()
        for s in self.zeroed:
            s.zero_()

    def backward(self, x, w):
        loss = (self.model(x).float() * w).sum()
        loss.backward()
        return loss.detach()


def model_inputs(n):
    g = torch.Generator(device="cuda").manual_seed(23)
    xs = [torch.randn(BS, SEQ, HID, device="cuda", generator=g).to(BF) for _ in range(n)]
    return xs, torch.randn(BS, SEQ, HID, device="cuda", generator=g)


def run_arm(monkeypatch, batched, twice=False, per_zero=1):
    """Loss bits and flat gradient buffer after each of three passes."""
    arm = Arm(monkeypatch, batched, twice)
    xs, w = model_inputs(3 * per_zero)
    out = []
    for i in range(3):
        arm.zero_grad()
        for j, x in enumerate(xs[i * per_zero:(i + 1) * per_zero]):
            torch.manual_seed(100 + 10 * i + j)       # the dropout masks
            loss = arm.backward(x, w)
            assert arm.owner.pending == [], "flushed when backward() returns"
        torch.cuda.synchronize()
        out.append((loss.clone(), arm.flat.clone()))
    return arm, out


def assert_same_run(on, off):
    for (la, fa), (lb, fb) in zip(on, off):
        assert torch.equal(la.view(1).view(torch.int32), lb.view(1).view(torch.int32))
        assert torch.equal(bits(fa), bits(fb))
    assert not torch.equal(bits(on[0][1]), bits(on[1][1])), "inputs differ per pass"


@pytest.mark.parametrize("twice,per_zero", [(False, 1), (False, 2), (True, 1)],
                         ids=["plain", "accumulate", "module_twice"])
def test_model_equal_on_and_off(monkeypatch, twice, per_zero):
    ref, off = run_arm(monkeypatch, False, twice, per_zero)
    arm, on = run_arm(monkeypatch, True, twice, per_zero)
    assert_same_run(on, off)
    assert ref.sites == [], "switch off: torch's pair"
    # Five sites a pass.  A layer run twice: its output LayerNorm finds its own
    # pending source, materialises it and folds; the Linear before it then
    # flushes mid-pass (its bias has a pending column sum) with three sources
    # left, and the two LayerNorms after that flush defer anew.
    assert arm.sites == ([3, 2] if twice else [5]) * (3 * per_zero)


def test_pending_entries_hold_sources(monkeypatch):
    from oktopk_amd.ops.fused_linear import LnGradSource

    arm = Arm(monkeypatch, True)
    xs, w = model_inputs(1)
    seen = []
    flush = arm.owner.flush

    def spy():
        seen.append(list(arm.owner.pending))
        flush()
    arm.owner.flush = spy
    arm.zero_grad()
    arm.backward(xs[0], w)
    ln = [e for e in seen[0] if not e[2]]
    assert len(ln) == 10 and all(isinstance(e[0], LnGradSource) for e in ln)


def test_references_dropped_after_flush(monkeypatch):
    arm = Arm(monkeypatch, True)
    xs, w = model_inputs(2)
    arm.zero_grad()
    arm.backward(xs[0], w)                 # first use: caches, workspaces
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    arm.zero_grad()
    arm.backward(xs[1], w)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert arm.sites == [5, 5]


def graph_run(monkeypatch, batched, xs, w):
    arm = Arm(monkeypatch, batched)
    static_x = xs[0].clone()
    torch.manual_seed(7)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            arm.zero_grad()
            arm.backward(static_x, w)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        arm.zero_grad()
        static_loss = arm.backward(static_x, w)
    assert arm.owner.pending == []
    out = []
    for x in xs:
        arm.flat.fill_(3.0)                    # replay must rewrite every slot
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        out.append((static_loss.clone(), arm.flat.clone()))
    return arm, out


def test_model_graph_replay(monkeypatch):
    """Three replays of the captured pass, switch on against switch off, same
    generator history; the launch is part of the graph."""
    xs, w = model_inputs(3)
    _, off = graph_run(monkeypatch, False, xs, w)
    arm, on = graph_run(monkeypatch, True, xs, w)
    assert_same_run(on, off)
    assert arm.sites == [5, 5, 5]              # two warm-up passes, one capture
