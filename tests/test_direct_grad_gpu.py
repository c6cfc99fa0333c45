"""Direct-gradient Linear backward: gW / gb written straight into gradient
slots (ops/csrc/direct_grad.hip, bindings linear_bwd_into, the autograd node
in ops/fused_linear.py and FlatBertAdam's slot ownership).

Tolerance, used everywhere below and derived rather than tuned:

    |got - ref| <= 2^-8 |ref| + L * 2^-24 * (|a|^T |b|)

ref is the fp32 result from the same bf16 operands.  The first term is one
bf16 rounding of the result; the second the worst-case fp32 accumulation
error of a length-L reduction, taken on the absolute-value product of the
operands.  An accumulated destination adds its previous content as one more
addend (L + 1, |prev| added to the product).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def hip():
    from oktopk_amd import _hip_ops

    return _hip_ops


def _asym(shape, seed, lo=-0.5, hi=1.5):
    """Asymmetric (non-zero-mean) random bf16 operand."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(BF).cuda()


def _bound(ref, L, absprod):
    return 2.0 ** -8 * ref.abs() + L * 2.0 ** -24 * absprod


def _assert_within(got, ref, L, absprod, what, scale=1.0):
    err = (got.float() - ref).abs()
    tol = scale * _bound(ref, L, absprod)
    ratio = (err / tol.clamp_min(1e-30)).max().item()
    print(f"{what}: max err/tol = {ratio:.3f}")
    assert bool((err <= tol).all()), f"{what}: max err/tol = {ratio:.3f}"


def _slot(numel, offset, seed):
    """A garbage-filled buffer and the [offset, offset+numel) slice of it."""
    g = torch.Generator().manual_seed(seed)
    buf = (torch.randn(numel + 64, generator=g) * 100.0).to(BF).cuda()
    return buf, buf[offset:offset + numel]


LINEAR_SHAPES = [(8, 32, 16), (130, 96, 200), (1024, 64, 2), (257, 40, 1002)]


def _check_linear_bwd_into(gy, x, w, offset, accumulate, seed):
    # both bias paths: torch's reduction into the slot (default) and the
    # one-launch column-sum kernel
    for bias_kernel in (False, True):
        _check_linear_bwd_into_1(gy, x, w, offset, accumulate, seed, bias_kernel)


def _check_linear_bwd_into_1(gy, x, w, offset, accumulate, seed, bias_kernel):
    N, K = w.shape
    gy2 = gy.reshape(-1, N).float()
    x2 = x.reshape(-1, K).float()
    R = gy2.shape[0]
    wbuf, wslot = _slot(N * K, offset, seed + 1)
    bbuf, bslot = _slot(N, offset, seed + 2)
    if accumulate:  # a known tensor instead of garbage
        wslot.copy_(_asym((N * K,), seed + 3, -1.0, 2.0))
        bslot.copy_(_asym((N,), seed + 4, -1.0, 2.0))
    wbuf0, bbuf0 = wbuf.clone(), bbuf.clone()
    pw = wslot.float().view(N, K) if accumulate else torch.zeros(N, K, device="cuda")
    pb = bslot.float().clone() if accumulate else torch.zeros(N, device="cuda")

    gx = hip().linear_bwd_into(gy, x, w, wslot.view(N, K), bslot, accumulate,
                               bias_kernel)

    assert gx.shape == x.shape and gx.dtype == BF
    _assert_within(gx.reshape(-1, K), gy2 @ w.float(), N,
                   gy2.abs() @ w.float().abs(), "gx")
    extra = 1 if accumulate else 0
    _assert_within(wslot.view(N, K), pw + gy2.t() @ x2, R + extra,
                   gy2.abs().t() @ x2.abs() + pw.abs(), "gW")
    _assert_within(bslot, pb + gy2.sum(0), R + extra,
                   gy2.abs().sum(0) + pb.abs(), "gb")
    # nothing around the destinations was touched
    for buf, buf0, n in ((wbuf, wbuf0, N * K), (bbuf, bbuf0, N)):
        assert torch.equal(buf[:offset], buf0[:offset])
        assert torch.equal(buf[offset + n:], buf0[offset + n:])


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("offset", [8, 3])
@pytest.mark.parametrize("R,K,N", LINEAR_SHAPES)
def test_linear_bwd_into(R, K, N, offset, accumulate):
    seed = R * 7 + N
    gy = _asym((R, N), seed)
    x = _asym((R, K), seed + 10, -1.0, 0.5)
    w = _asym((N, K), seed + 20, -0.25, 0.75)
    _check_linear_bwd_into(gy, x, w, offset, accumulate, seed)


@pytest.mark.parametrize("accumulate", [False, True])
def test_linear_bwd_into_3d_input(accumulate):
    gy = _asym((3, 43, 200), 5)
    x = _asym((3, 43, 96), 6, -1.0, 0.5)
    w = _asym((200, 96), 7, -0.25, 0.75)
    _check_linear_bwd_into(gy, x, w, 5, accumulate, 99)


# every column-sum variant: 16-byte vectors (C % 8 == 0), narrow C, 4-byte
# pairs (even C, the 30522 vocabulary), scalar (odd C), more rows than one
# block step, fewer rows than one
COLSUM_SHAPES = [(1024, 2), (1024, 768), (7, 768), (300, 2304), (515, 3072),
                 (64, 30522), (33, 1001), (5, 24), (9, 10), (1, 64), (600, 66)]


@pytest.mark.parametrize("R,C", COLSUM_SHAPES)
def test_colsum_into_matches_fp32_and_is_deterministic(R, C):
    gy = _asym((R, C), R + C)
    ref = gy.float().sum(0)
    absprod = gy.float().abs().sum(0)
    for offset in (8, 3):
        buf, dst = _slot(C, offset, C)
        buf0 = buf.clone()
        hip().colsum_bf16_into(gy, dst, False)
        _assert_within(dst, ref, R, absprod, f"colsum off{offset}")
        assert torch.equal(buf[:offset], buf0[:offset])
        assert torch.equal(buf[offset + C:], buf0[offset + C:])
        first = dst.clone()
        dst.fill_(7.0)
        hip().colsum_bf16_into(gy, dst, False)
        assert torch.equal(first, dst), "two runs must give identical bits"
        prev = dst.float().clone()
        hip().colsum_bf16_into(gy, dst, True)
        _assert_within(dst, prev + ref, R + 1, absprod + prev.abs(),
                       f"colsum acc off{offset}")


def test_colsum_into_unaligned_source():
    """A contiguous gy that starts 2 bytes into its storage takes the
    narrower-load variants; same result."""
    R, C = 130, 768
    flat = _asym((R * C + 1,), 11)
    gy = flat[1:].view(R, C)
    dst = torch.empty(C, dtype=BF, device="cuda")
    hip().colsum_bf16_into(gy, dst, False)
    _assert_within(dst, gy.float().sum(0), R, gy.float().abs().sum(0), "colsum")


# ---------------------------------------------------------------------------
# the autograd node
# ---------------------------------------------------------------------------

def test_node_returns_ordinary_grads_without_a_slot_owner():
    """Parameters no FlatBertAdam bound (here: plain tensors under SGD, and
    a parameter whose binding went stale): ordinary returned gradients, and
    post-accumulate hooks fire."""
    from oktopk_amd.ops.fused_linear import (GradSlotOwner, _DirectGradLinear,
                                             bind_grad_slot)

    x = _asym((4, 33, 96), 1, -1.0, 0.5).requires_grad_(True)
    w = _asym((200, 96), 2, -0.25, 0.75).requires_grad_(True)
    b = _asym((200,), 3).requires_grad_(True)
    fired = []
    w.register_post_accumulate_grad_hook(lambda p: fired.append("w"))
    b.register_post_accumulate_grad_hook(lambda p: fired.append("b"))
    opt = torch.optim.SGD([w, b], lr=0.1)
    # stale binding: the slot is not what .grad points at
    bind_grad_slot(w, torch.zeros_like(w), GradSlotOwner())
    gy = _asym((4, 33, 200), 4)
    _DirectGradLinear.apply(x, w, b, False).backward(gy)
    assert sorted(fired) == ["b", "w"]
    x2, w2, b2 = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    F.linear(x2, w2, b2).backward(gy)
    gy2, xf = gy.reshape(-1, 200).float(), x.detach().reshape(-1, 96).float()
    assert w.grad.shape == w2.grad.shape and b.grad.shape == b2.grad.shape
    _assert_within(x.grad.reshape(-1, 96), gy2 @ w.detach().float(), 200,
                   gy2.abs() @ w.detach().float().abs(), "gx")
    _assert_within(w.grad, gy2.t() @ xf, 132, gy2.abs().t() @ xf.abs(), "gW")
    _assert_within(b.grad, gy2.sum(0), 132, gy2.abs().sum(0), "gb")
    opt.step()


# ---------------------------------------------------------------------------
# module level, small BERT
# ---------------------------------------------------------------------------

SMALL = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2,
             intermediate_size=256, vocab_size=1000,
             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _trainer(monkeypatch, direct):
    from oktopk_amd.config import EngineConfig, OkTopkConfig
    from oktopk_amd.trainer import Trainer

    monkeypatch.setenv("OKTOPK_DIRECT_GRAD", "1" if direct else "0")
    torch.manual_seed(0)
    cfg = EngineConfig(compressor="oktopk", density=0.01,
                       oktopk=OkTopkConfig(dense_warmup_iters=0))
    tr = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg,
                 model_kwargs=SMALL, dtype="bf16")
    tr.batches.input_ids.clamp_(max=999)
    tr.batches.mlm_labels.clamp_(max=999)
    return tr


def _backward(tr, n_backwards=1, rec=None):
    """zero_grad + n backwards with the sub-step protocol; the loss is the
    model's own MLM + NSP loss, built here so that `rec` can see the logits'
    gradient.  Returns {name: fp32 grad}."""
    b, model = tr.batches, tr.model
    tr.opt.zero_grad()
    for sub in range(n_backwards):
        tr.opt.set_substep(sub)
        logits, nsp_logits = model(b.input_ids, token_type_ids=b.token_type,
                                   attention_mask=b.attn)
        if rec is not None:
            rec.watch_decoder(logits)
        loss = F.cross_entropy(logits.view(-1, logits.size(-1)),
                               b.mlm_labels.view(-1), ignore_index=-1)
        loss = loss + F.cross_entropy(nsp_logits.view(-1, 2), b.nsp.view(-1))
        loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.float().clone() for n, p in model.named_parameters()}


class _Operands:
    """Records, per parameter of the OFF arm, the reduction length L and the
    absolute-value operand product of its gradient (the tolerance's second
    term): Linear weight |gy|^T|x| and bias sum|gy| over R rows, LayerNorm
    gamma sum|gy * xhat| and beta sum|gy|, position / token-type embeddings
    the sum of |row gradients| they gather."""

    def __init__(self, model):
        from oktopk_amd.ops.fused_linear import ColsumLinear

        self.by_param = {}
        self.model = model
        for m in model.modules():
            if isinstance(m, ColsumLinear):
                m.register_forward_hook(self._linear)
            elif isinstance(m, torch.nn.LayerNorm):
                m.register_forward_hook(self._ln)
        model.transform_ln.register_forward_hook(self._decoder_in)
        emb = model.bert.embeddings
        emb.ln.register_forward_hook(self._emb)

    def _put(self, p, L, absprod):
        self.by_param[id(p)] = (L, absprod.reshape(p.shape))

    def _linear(self, m, inp, out):
        x = inp[0].detach()

        def on_grad(gy):
            g = gy.reshape(-1, gy.shape[-1]).float().abs()
            xa = x.reshape(-1, x.shape[-1]).float().abs()
            self._put(m.weight, g.shape[0], g.t() @ xa)
            self._put(m.bias, g.shape[0], g.sum(0))
        out.register_hook(on_grad)

    def _ln(self, m, inp, out):
        xhat = F.layer_norm(inp[0].detach().float(), m.normalized_shape, eps=m.eps)

        def on_grad(gy):
            g = gy.reshape(-1, gy.shape[-1]).float()
            self._put(m.weight, g.shape[0],
                      (g * xhat.reshape(g.shape)).abs().sum(0))
            self._put(m.bias, g.shape[0], g.abs().sum(0))
        out.register_hook(on_grad)

    def _decoder_in(self, m, inp, out):
        self.h = out.detach()

    def watch_decoder(self, logits):
        h = self.h
        emb = self.model.bert.embeddings.word_embeddings

        def on_grad(gy):
            g = gy.reshape(-1, gy.shape[-1]).float().abs()
            ha = h.reshape(-1, h.shape[-1]).float().abs()
            # the lookup's own gradient is the same kernel on the same input
            # in both arms and adds nothing to the allowance
            self._put(emb.weight, g.shape[0], g.t() @ ha)
            self._put(self.model.decoder_bias, g.shape[0], g.sum(0))
        logits.register_hook(on_grad)

    def _emb(self, m, inp, out):
        emb = self.model.bert.embeddings

        def on_grad(g):  # gradient of word + position + token-type sum
            ga = g.float().abs()                       # [B, S, H]
            B, S, H = ga.shape
            pos = torch.zeros_like(emb.position_embeddings.weight, dtype=torch.float32)
            pos[:S] = ga.sum(0)
            self._put(emb.position_embeddings.weight, B, pos)
            tt = ga.sum((0, 1)).expand_as(emb.token_type_embeddings.weight)
            self._put(emb.token_type_embeddings.weight, B * S, tt.contiguous())
        inp[0].register_hook(on_grad)


@pytest.fixture(scope="module")
def off_arm():
    """The reference arm (OKTOPK_DIRECT_GRAD=0), computed once and shared:
    gradients after one and after two backwards, and the operand record."""
    mp = pytest.MonkeyPatch()
    try:
        tr = _trainer(mp, direct=False)
        assert tr.opt._dg_owner is None and tr.opt._zero_ranges is None
        rec = _Operands(tr.model)
        once = _backward(tr, 1, rec)
        twice = _backward(tr, 2)
    finally:
        mp.undo()
    names = {id(p): n for n, p in tr.model.named_parameters()}
    ops = {names[k]: v for k, v in rec.by_param.items()}
    assert set(ops) == set(once), set(once) - set(ops)
    return once, twice, ops


def _compare(got, ref, ops, scale):
    for name, r in ref.items():
        L, absprod = ops[name]
        _assert_within(got[name], r, L, absprod, name, scale)


def test_bert_grads_match_off_arm(off_arm, monkeypatch):
    once, twice, ops = off_arm
    tr = _trainer(monkeypatch, direct=True)
    # every Linear weight/bias, the decoder bias and the tied word embedding
    # are bound: 4 Linears x 2 layers + pooler, transform, nsp = 11 Linears
    assert len(tr.opt._dg_params) == 11 * 2 + 2
    assert len(tr.opt._zero_ranges) == 2
    # poison the buffer: owned slots must be overwritten, the rest zeroed
    tr.opt.flat_grad_model.fill_(1000.0)
    got = _backward(tr, 1)
    _compare(got, once, ops, 1.0)
    # stronger than the bound: the default path runs the same GEMM and the
    # same reduction with another output pointer, so the bits are the same
    for name, r in once.items():
        assert torch.equal(got[name], r), f"{name} is not bit-identical"
    assert len(tr.opt._dg_params) == 24  # nothing fell back
    # two backwards without zero_grad: first overwrites, second accumulates
    tr.opt.flat_grad_model.fill_(-1000.0)
    _compare(_backward(tr, 2), twice, ops, 2.0)


def test_bert_unwritten_slot_falls_back(monkeypatch):
    """A backward that skips a bound module (MLM-only loss: pooler and NSP
    head unused) must not leave stale gradients: the optimizer zeroes those
    slots and returns them to zero + accumulate."""
    tr = _trainer(monkeypatch, direct=True)
    tr.opt.flat_grad_model.fill_(1000.0)
    tr.opt.zero_grad()
    b = tr.batches
    loss = tr.model(b.input_ids, token_type_ids=b.token_type,
                    attention_mask=b.attn, masked_lm_labels=b.mlm_labels)
    loss.backward()
    tr.opt.step()
    assert len(tr.opt._dg_params) == 24 - 4
    for m in (tr.model.bert.pooler, tr.model.nsp):
        assert float(m.weight.grad.abs().max()) == 0.0
        assert float(m.bias.grad.abs().max()) == 0.0


def test_bert_graph_replay_is_deterministic(monkeypatch):
    tr = _trainer(monkeypatch, direct=True)
    tr.step()
    assert tr.capture_graph()
    grads = []
    for _ in range(2):
        tr.opt.flat_grad_model.fill_(1000.0)
        tr.opt.zero_grad()
        tr._graph.replay()
        torch.cuda.synchronize()
        grads.append(tr.opt.flat_grad_model.clone())
    assert torch.equal(grads[0], grads[1])
    assert bool(torch.isfinite(grads[0].float()).all())
    assert float(grads[0].float().abs().max()) < 1000.0
