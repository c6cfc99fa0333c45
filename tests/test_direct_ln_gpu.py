"""LayerNorm backward writing the gamma/beta gradients into gradient slots
(ops/csrc/ln_bwd.hip, bindings ln_bwd_into, ops/slot_ln.py).

Reference: fp32 math on the same bf16 inputs and the same fp32 mean / rstd.
Tolerance form as in test_direct_grad_gpu.py,

    |got - ref| <= 2^-8 |ref| + L * 2^-24 * (|a|^T |b|)

with, per output:
  dgamma = sum_r gy * xhat   L = rows + 8, product sum_r |gy * xhat|
  dbeta  = sum_r gy          L = rows,     product sum_r |gy|
  gx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = gy * gamma
                             L = H + 8,    product rstd * (|g| + mean|g|
                                                   + |xhat| * mean|g * xhat|)
The + 8 covers the handful of fp32 roundings inside each addend (x - mean,
* rstd, * gy, * gamma, the final combination), each at most 2^-24 relative.
An accumulated slot adds its previous content as one more addend.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def hip():
    from oktopk_amd import _hip_ops

    return _hip_ops


def _asym(shape, seed, lo=-0.5, hi=1.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(BF).cuda()


def _within(got, ref, L, absprod, what):
    err = (got.float() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + L * 2.0 ** -24 * absprod
    ratio = (err / tol.clamp_min(1e-30)).max().item()
    print(f"{what}: max err/tol = {ratio:.3f}")
    assert bool((err <= tol).all()), f"{what}: max err/tol = {ratio:.3f}"


def _reference(gy, x, gamma, mean, rstd):
    gyf, xf, gf = gy.float(), x.float(), gamma.float()
    H = x.shape[-1]
    xhat = (xf - mean[:, None]) * rstd[:, None]
    g = gyf * gf
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * xhat).mean(-1, keepdim=True)
    gx = rstd[:, None] * (g - c1 - xhat * c2)
    gx_abs = rstd[:, None] * (g.abs() + g.abs().mean(-1, keepdim=True)
                              + xhat.abs() * (g * xhat).abs().mean(-1, keepdim=True))
    return dict(gx=gx, gx_abs=gx_abs, dg=(gyf * xhat).sum(0),
                dg_abs=(gyf * xhat).abs().sum(0), db=gyf.sum(0),
                db_abs=gyf.abs().sum(0), H=H)


LN_SHAPES = [(1, 128), (5, 768), (37, 256), (1023, 768), (1024, 1024)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("offset", [8, 3])
@pytest.mark.parametrize("rows,H", LN_SHAPES)
def test_ln_bwd_into(rows, H, offset, accumulate):
    assert hip().ln_bwd_supported(H)
    seed = rows + H
    gy = _asym((rows, H), seed)
    x = _asym((rows, H), seed + 1, -1.0, 3.0)
    # gamma itself sits at an odd element offset, as in the flat buffer
    gamma = _asym((H + 1,), seed + 2, 0.5, 1.5)[1:]
    xf = x.float()
    mean = xf.mean(-1)
    rstd = (xf.var(-1, unbiased=False) + 1e-12).rsqrt()
    ref = _reference(gy, x, gamma, mean, rstd)

    g = torch.Generator().manual_seed(seed + 3)
    buf = (torch.randn(2 * H + 64, generator=g) * 100.0).to(BF).cuda()
    dg = buf[offset:offset + H]
    db = buf[offset + H + 1:offset + 2 * H + 1]   # one element gap between
    if accumulate:
        dg.copy_(_asym((H,), seed + 4, -1.0, 2.0))
        db.copy_(_asym((H,), seed + 5, -1.0, 2.0))
    buf0 = buf.clone()
    pg = dg.float().clone() if accumulate else torch.zeros(H, device="cuda")
    pb = db.float().clone() if accumulate else torch.zeros(H, device="cuda")

    gx = hip().ln_bwd_into(gy, x, gamma, mean, rstd, dg, db, accumulate)

    extra = 1 if accumulate else 0
    _within(gx, ref["gx"], H + 8, ref["gx_abs"], "gx")
    _within(dg, pg + ref["dg"], rows + 8 + extra, ref["dg_abs"] + pg.abs(), "dgamma")
    _within(db, pb + ref["db"], rows + extra, ref["db_abs"] + pb.abs(), "dbeta")
    assert torch.equal(buf[:offset], buf0[:offset])
    assert torch.equal(buf[offset + H:offset + H + 1], buf0[offset + H:offset + H + 1])
    assert torch.equal(buf[offset + 2 * H + 1:], buf0[offset + 2 * H + 1:])
    if not accumulate:
        first = (gx.clone(), dg.clone(), db.clone())
        gx2 = hip().ln_bwd_into(gy, x, gamma, mean, rstd, dg, db, False)
        assert torch.equal(first[0], gx2) and torch.equal(first[1], dg) \
            and torch.equal(first[2], db), "two runs must give identical bits"


def _bound_ln(H, offset=3):
    from oktopk_amd.ops.fused_linear import GradSlotOwner, bind_grad_slot
    from oktopk_amd.ops.slot_ln import SlotLayerNorm

    ln = SlotLayerNorm(H, eps=1e-12).to(BF).cuda()
    with torch.no_grad():
        ln.weight.copy_(_asym((H,), 1, 0.5, 1.5))
        ln.bias.copy_(_asym((H,), 2))
    buf = torch.full((2 * H + 16,), 500.0, dtype=BF, device="cuda")
    owner = GradSlotOwner()
    ln.weight.grad = buf[offset:offset + H]
    ln.bias.grad = buf[offset + H:offset + 2 * H]
    bind_grad_slot(ln.weight, ln.weight.grad, owner)
    bind_grad_slot(ln.bias, ln.bias.grad, owner)
    return ln, owner


@pytest.mark.parametrize("H", [768, 96])
def test_slot_layernorm_module_matches_torch(H):
    """Bound SlotLayerNorm against nn.LayerNorm's own autograd on the same
    inputs: H = 768 runs the kernels (slots overwritten, then accumulated on
    a second backward), H = 96 is unsupported and falls back to torch's
    backward with ordinary gradients accumulated by autograd."""
    ln, owner = _bound_ln(H)
    if H == 96:  # the fallback accumulates: start from zero like zero_grad()
        ln.weight.grad.zero_()
        ln.bias.grad.zero_()
    x = _asym((4, 33, H), 3, -1.0, 3.0).requires_grad_(True)
    gy = _asym((4, 33, H), 4)
    y = ln(x)
    y.backward(gy)
    assert (len(owner.written) == 2) == bool(hip().ln_bwd_supported(H))

    ref_ln = torch.nn.LayerNorm(H, eps=1e-12).to(BF).cuda()
    with torch.no_grad():
        ref_ln.weight.copy_(ln.weight)
        ref_ln.bias.copy_(ln.bias)
    x2 = x.detach().clone().requires_grad_(True)
    y2 = ref_ln(x2)
    assert torch.equal(y, y2)
    y2.backward(gy)
    xf = x.detach().float().reshape(-1, H)
    mean = xf.mean(-1)
    rstd = (xf.var(-1, unbiased=False) + 1e-12).rsqrt()
    ref = _reference(gy.reshape(-1, H), x.detach().reshape(-1, H), ln.weight.detach(),
                     mean, rstd)
    rows = xf.shape[0]
    _within(x.grad.reshape(-1, H), ref["gx"], H + 8, ref["gx_abs"], "gx")
    _within(ln.weight.grad, ref["dg"], rows + 8, ref["dg_abs"], "dgamma")
    _within(ln.bias.grad, ref["db"], rows, ref["db_abs"], "dbeta")
    if H == 768:
        prev_g, prev_b = ln.weight.grad.float().clone(), ln.bias.grad.float().clone()
        ln(x).backward(gy)   # no zero_grad in between: accumulates
        _within(ln.weight.grad, prev_g + ref["dg"], rows + 9,
                ref["dg_abs"] + prev_g.abs(), "dgamma acc")
        _within(ln.bias.grad, prev_b + ref["db"], rows + 1,
                ref["db_abs"] + prev_b.abs(), "dbeta acc")


def test_bert_direct_ln_binds_and_overwrites(monkeypatch):
    """OKTOPK_DIRECT_LN=1 on the small BERT: the LayerNorm parameters are
    bound as well, a backward from a poisoned buffer leaves no poison and
    nothing falls back, and graph replay is deterministic."""
    from oktopk_amd.config import EngineConfig, OkTopkConfig
    from oktopk_amd.trainer import Trainer

    monkeypatch.setenv("OKTOPK_DIRECT_GRAD", "1")
    monkeypatch.setenv("OKTOPK_DIRECT_LN", "1")
    torch.manual_seed(0)
    kw = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2,
              intermediate_size=256, vocab_size=1000,
              hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg = EngineConfig(compressor="oktopk", density=0.01,
                       oktopk=OkTopkConfig(dense_warmup_iters=0))
    tr = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg,
                 model_kwargs=kw, dtype="bf16")
    tr.batches.input_ids.clamp_(max=999)
    tr.batches.mlm_labels.clamp_(max=999)
    assert len(tr.opt._dg_params) == 24 + 12   # 6 LayerNorms x (gamma, beta)
    tr.opt.flat_grad_model.fill_(1000.0)
    loss0 = tr.step()
    assert len(tr.opt._dg_params) == 36
    assert loss0 == loss0
    assert tr.capture_graph()
    grads = []
    for _ in range(2):
        tr.opt.flat_grad_model.fill_(1000.0)
        tr.opt.zero_grad()
        tr._graph.replay()
        torch.cuda.synchronize()
        grads.append(tr.opt.flat_grad_model.clone())
    assert torch.equal(grads[0], grads[1])
    assert float(grads[0].float().abs().max()) < 1000.0
