"""Fused residual LayerNorm kernels (ops/csrc/residual_ln.hip) against the
torch composition they stand in for, bit for bit.

Forward composition: native_dropout -> add -> native_layer_norm.  Backward:
gy1 + gy2 -> native_layer_norm_backward -> native_dropout_backward.  gamma and
beta sit at a 2-byte offset, as parameters aliased into a flat buffer may, so
that torch runs RowwiseMomentsCUDAKernel + LayerNormForwardCUDAKernel (with
everything 8-byte aligned it runs its vectorised kernel, which the fused path
leaves to torch).  NaN is required where torch yields NaN, equal bits
everywhere else.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 1e-12


@pytest.fixture(scope="module")
def hip():
    from oktopk_amd import _hip_ops

    return _hip_ops


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    it = torch.int16 if a.element_size() == 2 else torch.int32
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(nan_a, nan_b)) and bool(
        torch.equal(a.view(it)[~nan_a], b.view(it)[~nan_b]))


def affine(H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.randn(2 * H + 8, device="cuda", generator=g).to(BF)
    gamma, beta = buf[1:1 + H], buf[H + 3:2 * H + 3]
    gamma[::7] = 0
    gamma[1::5] *= -1
    assert gamma.data_ptr() % 8 and gamma.is_contiguous()
    return gamma, beta


def data(rows, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, H, device="cuda", generator=g)
    a = torch.randn(rows, H, device="cuda", generator=g)
    gy1 = torch.randn(rows, H, device="cuda", generator=g)
    gy2 = torch.randn(rows, H, device="cuda", generator=g)
    if rows >= 3:
        x[1] *= 1e4          # large magnitudes
        a[1] *= 1e4
        gy1[1] *= 1e-39      # subnormal gradients
        gy2[1] *= 1e-39
        x[2] = 0.5           # a row of equal values: variance 0
        a[2] = 0
    else:
        x[0, : H // 2] *= 1e4
    return x.to(BF), a.to(BF), gy1.to(BF), gy2.to(BF)


def reference(x, a, gy1, gy2, gamma, beta, p, train):
    H = x.shape[-1]
    mask = None
    d = a
    if train and p > 0:
        torch.manual_seed(5)
        d, mask = torch.native_dropout(a, p, True)
    s = x + d
    y, mean, rstd = torch.native_layer_norm(s, (H,), gamma, beta, EPS)
    gy = gy1 + gy2 if gy2 is not None else gy1
    gs, gw, gb = torch.ops.aten.native_layer_norm_backward(
        gy, s, [H], mean, rstd, gamma, beta, [True, True, True])
    ga = gs
    if mask is not None:
        ga = torch.ops.aten.native_dropout_backward(gs, mask, 1.0 / (1.0 - p))
    return dict(d=d, mask=mask, s=s, y=y, mean=mean.view(-1), rstd=rstd.view(-1),
                gy=gy, gs=gs, ga=ga, gw=gw, gb=gb)


@pytest.mark.parametrize("H", [768, 1024])
@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("p,train", [(0.1, True), (0.0, True), (0.1, False)],
                         ids=["p0.1", "p0", "eval"])
def test_kernels_match_torch_bits(hip, rows, H, p, train):
    from oktopk_amd.ops.residual_ln import torch_takes_rowwise_ln

    x, a, gy1, gy2 = data(rows, H, 100 + rows)
    gamma, beta = affine(H, 7)
    assert torch_takes_rowwise_ln(x, gamma, beta)
    ref = reference(x, a, gy1, gy2, gamma, beta, p, train)

    y, s, mean, rstd = hip.residual_ln_fwd(x, ref["d"], gamma, beta, EPS)
    for name, t in (("s", s), ("mean", mean), ("rstd", rstd), ("y", y)):
        assert same_bits(t, ref[name]), name

    scale = 1.0 / (1.0 - p)
    gy, gs, ga = hip.residual_ln_bwd(gy1, gy2, s, mean, rstd, gamma, ref["mask"], scale)
    for name, t in (("gy", gy), ("gs", gs), ("ga", ga)):
        assert same_bits(t, ref[name]), name
    # the single-gradient form, fed the sum
    gy_, gs1, ga1 = hip.residual_ln_bwd(ref["gy"], None, s, mean, rstd, gamma,
                                        ref["mask"], scale)
    assert gy_.data_ptr() == ref["gy"].data_ptr()
    assert same_bits(gs1, ref["gs"]) and same_bits(ga1, ref["ga"])


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("edges", [1, 2])
def test_autograd_function_matches_composition(p, edges):
    """Through autograd, with one or both of the two output edges used."""
    from oktopk_amd.ops.residual_ln import _ResidualLayerNormFn

    H, rows = 768, 64
    x, a, gy1, gy2 = data(rows, H, 3)
    if edges == 1:
        gy2 = None
    gamma, beta = affine(H, 13)
    ref = reference(x, a, gy1, gy2, gamma, beta, p, True)
    leaves = [t.clone().requires_grad_() for t in (x, a)]
    gl, bl = gamma.detach().requires_grad_(), beta.detach().requires_grad_()
    torch.manual_seed(5)
    y, edge = _ResidualLayerNormFn.apply(leaves[0], leaves[1], gl, bl, EPS, p, True)
    assert y.data_ptr() == edge.data_ptr()
    if edges == 2:
        torch.autograd.backward([y, edge], [gy1, gy2])
    else:
        edge.backward(gy1)
    assert same_bits(y.detach(), ref["y"])
    assert same_bits(leaves[0].grad, ref["gs"]) and same_bits(leaves[1].grad, ref["ga"])
    assert same_bits(gl.grad, ref["gw"]) and same_bits(bl.grad, ref["gb"])


# ---- model level: switch on against off ------------------------------------

SEQ, BS = 16, 2


class TinyBert(torch.nn.Module):
    def __init__(self, hidden=768, heads=12, p=0.1):
        super().__init__()
        from oktopk_amd.models.bert import BertConfig, BertLayer

        cfg = BertConfig(hidden_size=hidden, num_attention_heads=heads,
                         intermediate_size=4 * hidden, hidden_dropout_prob=p,
                         attention_probs_dropout_prob=p)
        self.layer = torch.nn.ModuleList(BertLayer(cfg) for _ in range(2))

    def forward(self, x):
        for lyr in self.layer:
            x = lyr(x, None)
        return x


class Arm:
    """Two BertLayers bound the way FlatBertAdam binds the model: parameters
    aliased into one bf16 buffer (the LayerNorm ones 4 bytes off an 8-byte
    boundary, as behind the flagship's decoder bias), .grad into a flat
    gradient buffer, Linear parameters owning their slots, LayerNorm slots
    zeroed and bound as add slots."""

    def __init__(self, monkeypatch, fused, p=0.1, dtype=BF, hidden=768, heads=12):
        from oktopk_amd import _hip_ops
        from oktopk_amd.ops import residual_ln
        from oktopk_amd.ops.fused_linear import (GradSlotOwner, bind_add_slot,
                                                 bind_grad_slot)
        from oktopk_amd.ops.slot_ln import SlotLayerNorm

        monkeypatch.setenv("OKTOPK_FUSED_RESIDUAL_LN", "1" if fused else "0")
        monkeypatch.setenv("OKTOPK_DEFER_SMALL_GRADS", "1")
        for k in ("OKTOPK_DIRECT_LN", "OKTOPK_COLSUM_BIAS"):
            monkeypatch.delenv(k, raising=False)
        torch.manual_seed(11)
        self.model = TinyBert(hidden, heads, p).to(dtype).cuda().train()
        ln_params = {id(q) for m in self.model.modules()
                     if isinstance(m, SlotLayerNorm) for q in m.parameters()}
        params = list(self.model.parameters())
        total = sum(q.numel() + 16 for q in params)
        self.flat_param = torch.zeros(total, dtype=dtype, device="cuda")
        self.flat = torch.zeros(total, dtype=dtype, device="cuda")
        self.owner = GradSlotOwner()
        self.zeroed = []
        off = 0
        with torch.no_grad():
            for q in params:
                off = (off + 7) // 8 * 8 + (2 if id(q) in ln_params else 0)
                n = q.numel()
                dst = self.flat_param[off:off + n].view_as(q)
                dst.copy_(q)
                if id(q) in ln_params and q.dim() == 1:
                    dst.add_(0.1 * torch.randn_like(dst))
                q.data = dst
                slot = self.flat[off:off + n].view_as(q)
                q.grad = slot
                if dtype == BF and id(q) not in ln_params:
                    bind_grad_slot(q, slot, self.owner)
                else:
                    self.zeroed.append(slot)
                    if dtype == BF:
                        bind_add_slot(q, slot, self.owner)
                off += n
        self.fwd_calls, self.bwd_edges, self.ln_adds = 0, [], 0
        real_fwd, real_bwd = residual_ln.residual_dropout_ln, _hip_ops.residual_ln_bwd
        real_flush = self.owner.flush

        def fwd(*a, **k):
            self.fwd_calls += 1
            return real_fwd(*a, **k)

        def bwd(gy1, gy2, *a):
            self.bwd_edges.append(1 if gy2 is None else 2)
            return real_bwd(gy1, gy2, *a)

        def flush():
            self.ln_adds += sum(1 for e in self.owner.pending if not e[2])
            real_flush()

        monkeypatch.setattr(residual_ln, "residual_dropout_ln", fwd)
        monkeypatch.setattr(_hip_ops, "residual_ln_bwd", bwd)
        self.owner.flush = flush

    def zero_grad(self):
        self.owner.discard()
        self.owner.written.clear()
        for s in self.zeroed:
            s.zero_()

    def backward(self, x, w):
        loss = (self.model(x).float() * w).sum()
        loss.backward()
        return loss.detach()


def model_inputs(n, hidden=768, dtype=BF):
    g = torch.Generator(device="cuda").manual_seed(23)
    xs = [torch.randn(BS, SEQ, hidden, device="cuda", generator=g).to(dtype)
          for _ in range(n)]
    return xs, torch.randn(BS, SEQ, hidden, device="cuda", generator=g)


def run_arm(monkeypatch, fused, per_zero=1, **kw):
    """Loss bits and flat gradient buffer after each of three passes."""
    arm = Arm(monkeypatch, fused, **kw)
    xs, w = model_inputs(3 * per_zero, kw.get("hidden", 768), kw.get("dtype", BF))
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
        assert same_bits(la.view(1), lb.view(1))
        assert same_bits(fa, fb)
    assert not same_bits(on[0][1], on[1][1]), "inputs differ per pass"


@pytest.mark.parametrize("per_zero", [1, 2], ids=["plain", "accumulate"])
def test_model_equal_on_and_off(monkeypatch, per_zero):
    _, off = run_arm(monkeypatch, False, per_zero)
    arm, on = run_arm(monkeypatch, True, per_zero)
    assert_same_run(on, off)
    passes = 3 * per_zero
    # all four sites fused; the last one has a single gradient edge; the
    # eight gamma / beta gradients went through the deferred add slots
    assert arm.fwd_calls == 4 * passes
    assert sorted(arm.bwd_edges) == [1] * passes + [2] * (3 * passes)
    assert arm.ln_adds == 8 * passes


@pytest.mark.parametrize("hidden,heads,dtype", [(640, 10, BF), (768, 12, torch.float32)],
                         ids=["H640", "fp32"])
def test_unsupported_model_takes_todays_path(monkeypatch, hidden, heads, dtype):
    """Forward and backward with the switch on give what the switch off
    gives, and no fused kernel runs."""
    kw = dict(hidden=hidden, heads=heads, dtype=dtype)
    _, off = run_arm(monkeypatch, False, **kw)
    arm, on = run_arm(monkeypatch, True, **kw)
    assert_same_run(on, off)
    assert arm.fwd_calls == 0 and arm.bwd_edges == []


def graph_run(monkeypatch, fused, p, xs, w):
    arm = Arm(monkeypatch, fused, p=p)
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
    xs, w = model_inputs(3)
    # with dropout: captured on against captured off, same generator history
    _, off = graph_run(monkeypatch, False, 0.1, xs, w)
    arm, on = graph_run(monkeypatch, True, 0.1, xs, w)
    assert_same_run(on, off)
    assert arm.fwd_calls == 4 * 3              # two warm-up passes, one capture
    # without dropout: three replays against the eager unfused passes
    eager = Arm(monkeypatch, False, p=0.0)
    want = []
    for x in xs:
        eager.flat.fill_(3.0)
        eager.zero_grad()
        want.append((eager.backward(x, w).clone(), eager.flat.clone()))
    _, got = graph_run(monkeypatch, True, 0.0, xs, w)
    assert_same_run(got, want)


def test_eligibility_switches_and_alignment(monkeypatch):
    from oktopk_amd.ops.residual_ln import residual_ln_available

    arm = Arm(monkeypatch, True)
    ln = arm.model.layer[0].ln1
    x = torch.randn(4, 768, device="cuda").to(BF)
    assert residual_ln_available(x, x.clone(), ln)
    monkeypatch.setenv("OKTOPK_DIRECT_LN", "1")
    assert not residual_ln_available(x, x.clone(), ln)
    monkeypatch.delenv("OKTOPK_DIRECT_LN")
    # aligned gamma and beta: torch runs its vectorised kernel, so do we
    ln.weight.data = ln.weight.data.clone()
    ln.bias.data = ln.bias.data.clone()
    assert not residual_ln_available(x, x.clone(), ln)


def test_flagship_sites_are_eligible():
    """The gain rests on the flat parameter layout leaving every LayerNorm
    parameter of BERT-base off 8-byte alignment; a layout change that ends it
    must fail here, not pass silently on the unfused path."""
    from oktopk_amd.config import EngineConfig
    from oktopk_amd.ops.residual_ln import residual_ln_available
    from oktopk_amd.trainer import Trainer

    cfg = EngineConfig.preset("bert", compressor="oktopk", density=0.001,
                              dense_warmup_iters=0)
    tr = Trainer(model_name="bert_base", batch_size=8, seq_len=128, cfg=cfg,
                 dtype="bf16")
    x = torch.randn(8, 128, 768, device="cuda").to(BF)
    layers = tr.model.bert.layer
    assert len(layers) == 12
    for lyr in layers:
        for ln in (lyr.ln1, lyr.ln2):
            assert residual_ln_available(x, x, ln)
