"""GPU numerics tests: HIP/CDNA4 kernels vs the fp32 torch reference.

Every op from oktopk_amd/ops/csrc is compared against
oktopk_amd/ops/reference.py on the same inputs (fp32).  Run on the MI355X
box: pytest tests -m gpu
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oktopk_amd.ops import reference as R


def hip():
    from oktopk_amd import _hip_ops

    return _hip_ops


def randn_gpu(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g).cuda()


@pytest.mark.parametrize("n,k", [(1000, 10), (100_000, 1000), (10_000_000, 10_000),
                                 (10_000_000, 100), (12_345_67, 1)])
def test_kth_abs_value_exact(n, k):
    t = randn_gpu(n, seed=n % 97)
    got = hip().kth_abs_value(t, k)
    want = torch.topk(t.abs(), k).values[-1].item()
    assert got == pytest.approx(want, rel=0, abs=0), (got, want)


def test_kth_abs_value_with_ties():
    t = torch.ones(10_000).cuda()
    t[::2] = 2.0
    assert hip().kth_abs_value(t, 100) == 2.0
    assert hip().kth_abs_value(t, 6000) == 1.0


@pytest.mark.parametrize("n", [1000, 1_000_000, 10_000_001])
@pytest.mark.parametrize("tau", [0.5, 2.0, 100.0])
def test_compact_gt_matches_reference(n, tau):
    t = randn_gpu(n, seed=int(tau * 10) + n % 13)
    gi, gv = hip().compact_gt(t, tau)
    ri, rv = R.compact_gt(t.cpu(), tau)
    assert gi.dtype == torch.int32
    assert torch.equal(gi.cpu(), ri)
    assert torch.equal(gv.cpu(), rv)
    if gi.numel() > 1:
        assert (gi[1:] > gi[:-1]).all()  # ascending (deterministic 2-pass)


def test_compact_gt_empty_and_full():
    t = randn_gpu(4096, seed=3)
    gi, gv = hip().compact_gt(t, 1e9)
    assert gi.numel() == 0 and gv.numel() == 0
    gi, gv = hip().compact_gt(t, -1.0)
    assert gi.numel() == 4096
    assert torch.equal(gv, t)


def test_count_gt():
    t = randn_gpu(1_000_000, seed=5)
    for tau in (0.0, 1.0, 3.0):
        assert hip().count_gt(t, tau) == R.count_gt(t.cpu(), tau)


def test_scatter_add_duplicates():
    dest = torch.zeros(1000).cuda()
    idx = torch.randint(0, 1000, (50_000,), dtype=torch.int32).cuda()
    val = torch.randn(50_000).cuda()
    hip().scatter_add_(dest, idx, val)
    ref = torch.zeros(1000)
    R.scatter_add_(ref, idx.cpu(), val.cpu())
    assert torch.allclose(dest.cpu(), ref, atol=1e-3)


def test_zero_at_and_fill_sparse():
    t = randn_gpu(1000, seed=7)
    idx = torch.tensor([0, 10, 999], dtype=torch.int32).cuda()
    hip().zero_at_(t, idx)
    assert t[idx.long()].abs().sum().item() == 0
    val = torch.tensor([1.0, 2.0, 3.0]).cuda()
    hip().fill_sparse_scaled_(t, idx, val, 0.5)
    assert t.cpu().sum().item() == pytest.approx(3.0)
    assert t[10].item() == 1.0


def test_isin_sorted():
    a = torch.tensor([3, 8, 15, 200, 5000], dtype=torch.int32).cuda()
    b = torch.tensor([8, 200, 10_000], dtype=torch.int32).cuda()
    got = hip().isin_sorted(a, b)
    assert got.cpu().tolist() == [False, True, False, True, False]


def test_ef_restore_snapshot():
    t = randn_gpu(1_000_003, seed=11)  # odd size exercises the scalar tail
    r = randn_gpu(1_000_003, seed=12)
    t_ref, r_ref = t.cpu().clone(), r.cpu().clone()
    hip().ef_restore_snapshot_(t, r)
    R.ef_restore_snapshot_(t_ref, r_ref)
    assert torch.equal(t.cpu(), t_ref)
    assert torch.equal(r.cpu(), r_ref)


def test_fused_sgd_matches_reference():
    p = randn_gpu(10_000, seed=20)
    g = randn_gpu(10_000, seed=21)
    buf = torch.zeros(10_000).cuda()
    p_ref, buf_ref = p.cpu().clone(), torch.zeros(10_000)
    for _ in range(3):
        hip().fused_sgd_(p, g, buf, 0.1, 0.9, 1e-4, True)
        R.fused_sgd_(p_ref, g.cpu(), buf_ref, 0.1, 0.9, 1e-4, True)
    assert torch.allclose(p.cpu(), p_ref, atol=1e-5)


def test_fused_adam_matches_reference():
    p = randn_gpu(10_000, seed=30)
    g = randn_gpu(10_000, seed=31)
    m = torch.zeros(10_000).cuda()
    v = torch.zeros(10_000).cuda()
    p_ref = p.cpu().clone()
    m_ref, v_ref = torch.zeros(10_000), torch.zeros(10_000)
    for _ in range(3):
        hip().fused_adam_(p, g, m, v, 1e-3, 0.9, 0.999, 1e-6, 0.01)
        R.fused_adam_(p_ref, g.cpu(), m_ref, v_ref, 1e-3, 0.9, 0.999, 1e-6, 0.01)
    assert torch.allclose(p.cpu(), p_ref, atol=1e-5)
    assert torch.allclose(v.cpu(), v_ref, atol=1e-6)


def test_l2norm():
    t = randn_gpu(5_000_000, seed=40)
    # kernel accumulates in fp64; compare against an fp64 host reference
    want = float(t.cpu().double().norm(p=2).item())
    assert hip().l2norm(t) == pytest.approx(want, rel=1e-10)


def test_engine_gpu_matches_cpu_world1():
    """Whole ok-topk pipeline, GPU (HIP kernels) vs CPU (torch reference)."""
    from oktopk_amd import AllReducer, Comm, EngineConfig
    from oktopk_amd.config import OkTopkConfig

    def build():
        return AllReducer(
            Comm(None),
            EngineConfig(compressor="oktopk", density=0.01,
                         oktopk=OkTopkConfig(dense_warmup_iters=0)),
        )

    eng_gpu, eng_cpu = build(), build()
    for it in range(4):
        g = torch.Generator().manual_seed(it)
        t = torch.randn(100_000, generator=g)
        out_gpu = eng_gpu.run("w", t.cuda()).cpu()
        out_cpu = eng_cpu.run("w", t.clone())
        assert torch.allclose(out_gpu, out_cpu, atol=1e-5), it
    assert torch.allclose(
        eng_gpu.states["w"].residual.cpu(), eng_cpu.states["w"].residual, atol=1e-5
    )


def test_trainer_smoke_gpu():
    from oktopk_amd.config import EngineConfig, OkTopkConfig
    from oktopk_amd.trainer import Trainer

    cfg = EngineConfig(compressor="oktopk", density=0.001,
                       oktopk=OkTopkConfig(dense_warmup_iters=0))
    tr = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg, dtype="bf16")
    l0 = tr.step()
    l1 = tr.step()
    assert l0 == l0 and l1 == l1


def test_fused_linear_gelu_forward():
    """MFMA fused GEMM+bias+GELU vs fp32 torch reference (asymmetric random
    operands catch operand/output transposes, HIP guide G9/rule 16)."""
    from oktopk_amd import _hip_ops

    torch.manual_seed(0)
    for M, N, K in [(1024, 3072, 768), (128, 128, 32), (100, 64, 64), (257, 192, 96)]:
        x = (torch.randn(M, K) * 0.5).bfloat16().cuda()
        w = (torch.randn(N, K) * 0.5).bfloat16().cuda()
        b = torch.randn(N).bfloat16().cuda()
        y, z = _hip_ops.linear_gelu(x, w, b, True, True)
        ref_pre = x.float() @ w.float().t() + b.float()
        ref = torch.nn.functional.gelu(ref_pre)
        assert torch.allclose(z.float(), ref_pre, atol=0.15, rtol=0.02), (
            (z.float() - ref_pre).abs().max()
        )
        err = (y.float() - ref).abs()
        tol = 0.05 + 0.02 * ref.abs()
        assert (err <= tol).float().mean() > 0.999, err.max()


def test_fused_linear_gelu_autograd():
    from oktopk_amd.ops.fused_linear import fused_linear_gelu

    torch.manual_seed(1)
    M, N, K = 256, 128, 64
    x = (torch.randn(M, K) * 0.5).bfloat16().cuda().requires_grad_(True)
    w = (torch.randn(N, K) * 0.5).bfloat16().cuda().requires_grad_(True)
    b = torch.randn(N).bfloat16().cuda().requires_grad_(True)
    y = fused_linear_gelu(x, w, b)
    gy = torch.randn_like(y)
    y.backward(gy)

    x2 = x.detach().float().requires_grad_(True)
    w2 = w.detach().float().requires_grad_(True)
    b2 = b.detach().float().requires_grad_(True)
    ref = torch.nn.functional.gelu(x2 @ w2.t() + b2)
    ref.backward(gy.float())
    assert torch.allclose(x.grad.float(), x2.grad, atol=0.3, rtol=0.05), (
        (x.grad.float() - x2.grad).abs().max()
    )
    assert torch.allclose(w.grad.float(), w2.grad, atol=0.5, rtol=0.05), (
        (w.grad.float() - w2.grad).abs().max()
    )


def test_bert_layer_uses_fused_mlp():
    """On GPU/bf16 the BertLayer MLP must run the MFMA kernel and match the
    torch path numerically."""
    import os
    from oktopk_amd.models.bert import BertConfig, BertLayer

    torch.manual_seed(2)
    cfg = BertConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    lyr = BertLayer(cfg).bfloat16().cuda()
    x = torch.randn(2, 16, 128).bfloat16().cuda()
    os.environ["OKTOPK_FUSED_MLP"] = "1"
    try:
        out_fused = lyr(x)
    finally:
        os.environ["OKTOPK_FUSED_MLP"] = "0"
    out_ref = lyr(x)
    assert torch.allclose(out_fused.float(), out_ref.float(), atol=0.1), (
        (out_fused - out_ref).abs().max()
    )


def test_zero_at_masked():
    t = randn_gpu(1000, seed=50)
    ref = t.cpu().clone()
    idx = torch.tensor([5, 100, 200, 999], dtype=torch.int32).cuda()
    mask = torch.zeros(1000, dtype=torch.bool).cuda()
    mask[100] = True
    mask[999] = True
    hip().zero_at_masked_(t, idx, mask)
    R.zero_at_masked_(ref, idx.cpu(), mask.cpu())
    assert torch.equal(t.cpu(), ref)
    assert t[100].item() == 0 and t[999].item() == 0 and t[5].item() != 0


def test_fused_add_layernorm_fwd_bwd():
    """Fused add+LN vs the unfused torch path: forward within bf16 rounding,
    backward gradients (input, gamma, beta) close to fp32 reference."""
    from oktopk_amd import _hip_ops

    torch.manual_seed(3)
    for rows, H in [(1024, 768), (100, 128), (37, 256)]:
        x = (torch.randn(rows, H) * 0.5).bfloat16().cuda()
        r = (torch.randn(rows, H) * 0.5).bfloat16().cuda()
        w = torch.randn(H).bfloat16().cuda()
        b = torch.randn(H).bfloat16().cuda()
        y, s, mean, rstd = _hip_ops.add_ln_fwd(x, r, w, b, 1e-12)
        s_ref = (x + r)  # bf16 sum, like the kernel materialises
        ref = torch.nn.functional.layer_norm(
            s_ref.float(), (H,), w.float(), b.float(), 1e-12
        )
        assert torch.equal(s, s_ref)
        assert torch.allclose(y.float(), ref, atol=0.05, rtol=0.02), (
            (y.float() - ref).abs().max()
        )
        # backward
        gy = torch.randn(rows, H).bfloat16().cuda()
        gx, dgamma, dbeta = _hip_ops.add_ln_bwd(gy, s, mean, rstd, w)
        sf = s.float().detach().requires_grad_(True)
        wf = w.float().detach().requires_grad_(True)
        bf = b.float().detach().requires_grad_(True)
        out = torch.nn.functional.layer_norm(sf, (H,), wf, bf, 1e-12)
        out.backward(gy.float())
        assert torch.allclose(gx.float(), sf.grad, atol=0.1, rtol=0.05), (
            (gx.float() - sf.grad).abs().max()
        )
        assert torch.allclose(dgamma, wf.grad, atol=0.2, rtol=0.02), (
            (dgamma - wf.grad).abs().max()
        )
        assert torch.allclose(dbeta, bf.grad, atol=0.2, rtol=0.02), (
            (dbeta - bf.grad).abs().max()
        )


def test_fused_add_layernorm_autograd_module():
    from oktopk_amd.ops.fused_ln import fused_add_layernorm

    torch.manual_seed(4)
    H = 128
    ln = torch.nn.LayerNorm(H).bfloat16().cuda()
    x = (torch.randn(4, 8, H)).bfloat16().cuda().requires_grad_(True)
    r = (torch.randn(4, 8, H)).bfloat16().cuda().requires_grad_(True)
    y = fused_add_layernorm(x, r, ln)
    y.sum().backward()
    assert torch.equal(x.grad, r.grad)  # add passes gradient through
    assert ln.weight.grad is not None and torch.isfinite(ln.weight.grad).all()


def _attn_ref(qkv, mask, nh, dropout_p=0.0):
    b, s, h3 = qkv.shape
    h = h3 // 3
    hd = h // nh
    q, k, v = (
        qkv.view(b, s, 3, nh, hd).permute(2, 0, 3, 1, 4).float().unbind(0)
    )
    scores = q @ k.transpose(-1, -2) / (hd ** 0.5)
    if mask is not None:
        scores = scores + mask.view(b, 1, 1, s).float()
    p = torch.softmax(scores, dim=-1)
    ctx = p @ v
    return ctx.transpose(1, 2).reshape(b, s, h), p


def test_fused_attention_forward_no_dropout():
    from oktopk_amd import _hip_ops

    torch.manual_seed(5)
    b, s, nh, hd = 3, 128, 4, 64
    qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16().cuda()
    mask = torch.zeros(b, s).bfloat16().cuda()
    mask[:, 100:] = -10000.0  # padded keys
    out, p, a = _hip_ops.attn_fwd(qkv, mask, nh, 0.0, True, True)
    ref, p_ref = _attn_ref(qkv, mask, nh)
    assert torch.allclose(out.float(), ref, atol=0.03, rtol=0.02), (
        (out.float() - ref).abs().max()
    )
    assert torch.allclose(
        p.view(b, nh, s, s).float(), p_ref, atol=0.01
    ), (p.view(b, nh, s, s).float() - p_ref).abs().max()
    assert torch.equal(p, a)  # no dropout -> identical


def test_fused_attention_dropout_stats():
    from oktopk_amd import _hip_ops

    torch.manual_seed(6)
    b, s, nh = 4, 128, 8
    qkv = (torch.randn(b, s, 3 * nh * 64) * 0.5).bfloat16().cuda()
    drop_p = 0.25
    out, p, a = _hip_ops.attn_fwd(qkv, torch.empty(0).cuda(), nh, drop_p, True, True)
    dropped = (a == 0) & (p != 0)
    frac = dropped.float().mean().item()
    assert abs(frac - drop_p) < 0.01, frac
    # kept entries are scaled by 1/keep
    kept = a != 0
    ratio = (a[kept].float() / p[kept].float()).mean().item()
    assert abs(ratio - 1 / (1 - drop_p)) < 0.02, ratio
    # two calls give different masks (generator offset advances)
    _, _, a2 = _hip_ops.attn_fwd(qkv, torch.empty(0).cuda(), nh, drop_p, True, True)
    assert not torch.equal(a, a2)


def test_fused_attention_autograd():
    from oktopk_amd.ops.fused_attn import fused_attention

    torch.manual_seed(7)
    b, s, nh, hd = 2, 128, 4, 64
    qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16().cuda().requires_grad_(True)
    mask = torch.zeros(b, s).bfloat16().cuda()
    out = fused_attention(qkv, mask, nh, 0.0, True)
    gy = torch.randn_like(out)
    out.backward(gy)

    q2 = qkv.detach().float().requires_grad_(True)
    ctxr, _ = _attn_ref(q2, mask, nh)
    ctxr.backward(gy.float())
    assert torch.allclose(qkv.grad.float(), q2.grad, atol=0.1, rtol=0.05), (
        (qkv.grad.float() - q2.grad).abs().max()
    )


def test_bert_layer_fused_attention_matches_eager():
    import os
    from oktopk_amd.models.bert import BertConfig, BertLayer

    torch.manual_seed(8)
    cfg = BertConfig(hidden_size=768, num_attention_heads=12,
                     intermediate_size=1024, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0)
    lyr = BertLayer(cfg).bfloat16().cuda()
    x = torch.randn(2, 128, 768).bfloat16().cuda()
    os.environ["OKTOPK_FUSED_ATTN"] = "1"
    try:
        out_fused = lyr(x)
    finally:
        os.environ["OKTOPK_FUSED_ATTN"] = "0"
    out_eager = lyr(x)
    assert torch.allclose(out_fused.float(), out_eager.float(), atol=0.12), (
        (out_fused.float() - out_eager.float()).abs().max()
    )


def test_checkpoint_resume_bf16_masters(tmp_path_factory):
    """Pure-bf16 path: resume must restore the fp32 MASTER weights, not just
    the bf16 model mirrors — otherwise the first post-resume step applies an
    update to the stale (random-init) master and destroys the loaded model."""
    from oktopk_amd.config import EngineConfig, OkTopkConfig
    from oktopk_amd.trainer import Trainer
    from oktopk_amd.utils import load_checkpoint, save_checkpoint

    tmp = tmp_path_factory.mktemp("ck")
    kw = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2,
              intermediate_size=256, vocab_size=1000)
    cfg = EngineConfig(compressor="oktopk", density=0.01,
                       oktopk=OkTopkConfig(dense_warmup_iters=0))
    tr = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg,
                 model_kwargs=kw, dtype="bf16")
    tr.batches.input_ids.clamp_(max=999)
    tr.batches.mlm_labels.clamp_(max=999)
    for _ in range(3):
        tr.step()
    path = str(tmp / "ck.pth")
    save_checkpoint(path, tr.model, tr.opt, iteration=3, epoch=0)
    w_saved = tr.opt.flat_param.clone()

    tr2 = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg,
                  model_kwargs=kw, dtype="bf16")
    tr2.batches.input_ids.clamp_(max=999)
    tr2.batches.mlm_labels.clamp_(max=999)
    load_checkpoint(path, tr2.model, tr2.opt)
    assert torch.allclose(tr2.opt.flat_param, w_saved)
    before = tr2.opt.flat_param.clone()
    tr2.step()
    delta = (tr2.opt.flat_param - before).abs().max().item()
    # one Adam step at lr 2e-4 moves weights by <= ~lr scale, not by the
    # distance between two random inits (~0.04)
    assert delta < 5e-3, delta


def test_fused_adam_mirror():
    for n in (10_000, 10_003):  # without / with a scalar tail (n % 4 != 0)
        p = randn_gpu(n, seed=60)
        g = randn_gpu(n, seed=61)
        m = torch.zeros(n).cuda()
        v = torch.zeros(n).cuda()
        pb = torch.zeros(n, dtype=torch.bfloat16).cuda()
        p_ref = p.clone()
        m_ref, v_ref = m.clone(), v.clone()
        hip().fused_adam_mirror_(p, g, m, v, pb, 1e-3, 0.9, 0.999, 1e-6, 0.01)
        hip().fused_adam_(p_ref, g, m_ref, v_ref, 1e-3, 0.9, 0.999, 1e-6, 0.01)
        assert torch.equal(p, p_ref)
        assert torch.equal(pb, p.to(torch.bfloat16))


@pytest.mark.parametrize("n", [1000, 109_482_240 // 16, 1_000_001])
@pytest.mark.parametrize("with_grad", [False, True])
def test_compact_adaptive_ef_matches_reference(n, with_grad):
    g = torch.Generator().manual_seed(n % 97)
    t_cpu = torch.randn(n, generator=g)
    r_cpu = torch.randn(n, generator=g) * 0.05
    grad_cpu = torch.randn(n, generator=g).bfloat16() if with_grad else None
    k = max(1, n // 1000)
    tau0 = R.kth_abs_value((grad_cpu.float() + r_cpu) if with_grad else (t_cpu + r_cpu), k)
    taus = [tau0 * 0.97 * 1.03 ** i for i in range(4)]

    t_g = t_cpu.cuda()
    r_g = r_cpu.cuda()
    grad_g = grad_cpu.cuda() if with_grad else None
    idx, val, chosen, cnt = hip().compact_adaptive_ef(
        t_g, r_g, grad_g, taus, 4 * k // 3)

    idx2, val2, chosen2, cnt2 = R.compact_adaptive_ef(
        t_cpu, r_cpu, grad_cpu, taus, 4 * k // 3)
    assert int(chosen) == chosen2 and int(cnt) == cnt2
    assert torch.equal(idx.cpu(), idx2)
    # a copied float and one fp32 add: no tolerance
    assert torch.equal(val.cpu(), val2)
    # contract: t is NOT written (the steady state never reads it back)
    assert torch.equal(t_g.cpu(), t_cpu)
    assert torch.equal(r_g.cpu(), r_cpu)


def test_engine_chunked_gpu_matches_cpu_world1():
    """Chunked engine (pipeline_chunks=3) on GPU vs CPU torch reference."""
    from oktopk_amd import AllReducer, Comm, EngineConfig
    from oktopk_amd.config import OkTopkConfig

    def build():
        return AllReducer(
            Comm(None),
            EngineConfig(compressor="oktopk", density=0.01,
                         oktopk=OkTopkConfig(dense_warmup_iters=0,
                                             pipeline_chunks=3)),
        )

    eng_gpu, eng_cpu = build(), build()
    for it in range(4):
        g = torch.Generator().manual_seed(it)
        t = torch.randn(100_001, generator=g)  # odd size: ragged last chunk
        out_gpu = eng_gpu.run("w", t.cuda()).cpu()
        out_cpu = eng_cpu.run("w", t.clone())
        assert torch.allclose(out_gpu, out_cpu, atol=1e-5), it
    for i in range(3):
        assert torch.allclose(eng_gpu.states[f"w/c{i}"].residual.cpu(),
                              eng_cpu.states[f"w/c{i}"].residual, atol=1e-5)


@pytest.mark.parametrize("comp", ["topkAopt", "topkSA", "gaussiank", "gtopk"])
def test_engine_baselines_gpu_match_cpu_world1(comp):
    """Baseline compressors, GPU (HIP kernels incl. fused EF+count where
    adopted) vs CPU torch reference."""
    from oktopk_amd import AllReducer, Comm, EngineConfig
    from oktopk_amd.config import OkTopkConfig

    def build():
        return AllReducer(
            Comm(None),
            EngineConfig(compressor=comp, density=0.01,
                         oktopk=OkTopkConfig(dense_warmup_iters=0)),
        )

    eng_gpu, eng_cpu = build(), build()
    for it in range(4):
        g = torch.Generator().manual_seed(100 + it)
        t = torch.randn(200_000, generator=g)
        out_gpu = eng_gpu.run("w", t.cuda()).cpu()
        out_cpu = eng_cpu.run("w", t.clone())
        assert torch.allclose(out_gpu, out_cpu, atol=1e-4), (comp, it)
    assert torch.allclose(eng_gpu.states["w"].residual.cpu(),
                          eng_cpu.states["w"].residual, atol=1e-4)


def test_model_variants_forward_backward_gpu():
    """Late-round model additions (preresnet/resnet_mod/mnistnet) run
    fwd+bwd on the GPU."""
    from oktopk_amd import models

    cases = [("preresnet20", (2, 3, 32, 32)), ("resnet_mod20", (2, 3, 32, 32)),
             ("mnistnet", (2, 1, 28, 28))]
    for name, shape in cases:
        m = models.create_net(name).cuda()
        y = m(torch.randn(*shape, device="cuda"))
        y.sum().backward()
        assert torch.isfinite(y).all(), name


# ---------------------------------------------------------------------------
# flash (online-softmax) attention — any seq % 128 == 0 (attention_fa.hip)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("s", [128, 256, 512])
def test_flash_attention_forward(s):
    from oktopk_amd import _hip_ops

    torch.manual_seed(11)
    b, nh, hd = 2, 4, 64
    qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16().cuda()
    mask = torch.zeros(b, s).bfloat16().cuda()
    mask[:, s - 17:] = -10000.0  # padded keys
    out, lse, _ = _hip_ops.attn_fwd_fa(qkv, mask, nh, 0.0, True, True)
    ref, p_ref = _attn_ref(qkv, mask, nh)
    assert torch.allclose(out.float(), ref, atol=0.03, rtol=0.02), (
        s, (out.float() - ref).abs().max())
    # LSE must match the reference softmax normaliser
    q, k, _ = (qkv.view(b, s, 3, nh, hd).permute(2, 0, 3, 1, 4).float()
               .unbind(0))
    scores = q @ k.transpose(-1, -2) / (hd ** 0.5) + mask.view(b, 1, 1, s).float()
    lse_ref = torch.logsumexp(scores, dim=-1).reshape(b * nh, s)
    assert torch.allclose(lse, lse_ref, atol=2e-2, rtol=1e-3), (
        (lse - lse_ref).abs().max())


def test_flash_attention_matches_legacy_seq128():
    """The online-softmax kernel must agree with the single-pass seq-128
    kernel (same MFMA structure, different softmax order)."""
    from oktopk_amd import _hip_ops

    torch.manual_seed(12)
    b, s, nh = 3, 128, 8
    qkv = (torch.randn(b, s, 3 * nh * 64) * 0.5).bfloat16().cuda()
    out_fa, _, _ = _hip_ops.attn_fwd_fa(
        qkv, torch.empty(0).cuda(), nh, 0.0, True, True)
    out_legacy = _hip_ops.attn_fwd(
        qkv, torch.empty(0).cuda(), nh, 0.0, True, False)[0]
    assert torch.allclose(out_fa.float(), out_legacy.float(),
                          atol=0.02, rtol=0.02), (
        (out_fa.float() - out_legacy.float()).abs().max())


def test_flash_attention_dropout_mask_regen():
    """The backward regenerates the forward's philox dropout mask exactly:
    apply dropout_mask_mul_ to the reference P and compare the zero set
    against the forward's dropped contributions."""
    from oktopk_amd import _hip_ops

    torch.manual_seed(13)
    b, s, nh, hd = 2, 256, 4, 64
    drop_p = 0.25
    qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16().cuda()
    out, lse, philox = _hip_ops.attn_fwd_fa(
        qkv, torch.empty(0).cuda(), nh, drop_p, True, True)
    # reference A from regenerated mask
    ref, p_ref = _attn_ref(qkv, torch.zeros(b, s).bfloat16().cuda(), nh)
    a = p_ref.reshape(b * nh, s, s).bfloat16().contiguous()
    _hip_ops.dropout_mask_mul_(a, philox, drop_p)
    dropped = ((a == 0) & (p_ref.reshape(b * nh, s, s).bfloat16() != 0))
    frac = dropped.float().mean().item()
    assert abs(frac - drop_p) < 0.01, frac
    # ctx from the regenerated A must equal the kernel's dropout output
    v = (qkv.view(b, s, 3, nh, hd).permute(2, 0, 3, 1, 4).float()
         .unbind(0))[2]
    ctx = (a.float().view(b, nh, s, s) @ v).transpose(1, 2).reshape(
        b, s, nh * hd)
    assert torch.allclose(out.float(), ctx, atol=0.06, rtol=0.05), (
        (out.float() - ctx).abs().max())


@pytest.mark.parametrize("s", [256, 512])
def test_flash_attention_autograd(s):
    from oktopk_amd.ops.fused_attn import _FlashAttention

    torch.manual_seed(14)
    b, nh, hd = 2, 4, 64
    qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16().cuda() \
        .requires_grad_(True)
    mask = torch.zeros(b, s).bfloat16().cuda()
    out = _FlashAttention.apply(qkv, mask, nh, 0.0, True)
    gy = torch.randn_like(out)
    out.backward(gy)

    q2 = qkv.detach().float().requires_grad_(True)
    ctxr, _ = _attn_ref(q2, mask, nh)
    ctxr.backward(gy.float())
    assert torch.allclose(qkv.grad.float(), q2.grad, atol=0.1, rtol=0.05), (
        (qkv.grad.float() - q2.grad).abs().max())


def test_flash_attention_spiked_key_rescale():
    """Force the online rescale across tiles: one huge key in the LAST
    tile makes every earlier tile's max stale, so the rescale path (not
    just the first-tile initialisation) is exercised (guide T13 test
    discipline: spike a K row so the running max grows late)."""
    from oktopk_amd import _hip_ops

    torch.manual_seed(15)
    b, s, nh, hd = 1, 384, 2, 64
    qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16()
    # spike: key row 300 parallel to every query -> dominates all scores
    qkv5 = qkv.view(b, s, 3, nh, hd)
    qkv5[:, 300, 1] = 4.0
    qkv5[:, :, 0, :, :] = qkv5[:, :, 0, :, :].abs()  # q . k_spike >> others
    qkv = qkv.cuda().contiguous()
    out, lse, _ = _hip_ops.attn_fwd_fa(
        qkv, torch.empty(0).cuda(), nh, 0.0, True, True)
    ref, _ = _attn_ref(qkv, None, nh)
    assert torch.allclose(out.float(), ref, atol=0.04, rtol=0.03), (
        (out.float() - ref).abs().max())


@pytest.mark.parametrize("s", [128, 256, 384])
def test_flash_attention_bwd_kernel_vs_torch_recompute(s):
    """The hand-written flash backward (attn_bwd_dq/_dkv) must match the
    torch-recompute backward (OKTOPK_ATTN_BWD_TORCH=1, itself validated
    against autograd above) including dropout — the philox mask regen
    must agree bit-for-bit between the two paths."""
    import os
    from oktopk_amd.ops.fused_attn import _FlashAttention

    for drop_p in (0.0, 0.2):
        grads = {}
        for mode in ("kernel", "torch"):
            torch.manual_seed(21)
            torch.cuda.manual_seed_all(21)
            b, nh, hd = 2, 4, 64
            qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16().cuda() \
                .requires_grad_(True)
            mask = torch.zeros(b, s).bfloat16().cuda()
            mask[:, s - 9:] = -10000.0
            os.environ["OKTOPK_ATTN_BWD_TORCH"] = \
                "1" if mode == "torch" else "0"
            try:
                out = _FlashAttention.apply(qkv, mask, nh, drop_p, True)
                gy = torch.randn(out.shape, generator=torch.Generator(
                    device="cuda").manual_seed(3), device="cuda").bfloat16()
                out.backward(gy)
            finally:
                os.environ["OKTOPK_ATTN_BWD_TORCH"] = "0"
            grads[mode] = qkv.grad.detach().float()
        diff = (grads["kernel"] - grads["torch"]).abs().max().item()
        ref = grads["torch"].abs().max().item()
        assert diff <= max(0.02, 0.02 * ref), (s, drop_p, diff, ref)


def test_flash_attention_bwd_dropout_autograd():
    """Full-chain dropout gradient: kernel fwd+bwd vs a torch fp32
    reference that uses the kernel's OWN regenerated dropout mask (the
    mask is the kernel's rng choice — the reference must adopt it)."""
    from oktopk_amd import _hip_ops
    from oktopk_amd.ops.fused_attn import _FlashAttention

    torch.manual_seed(22)
    b, s, nh, hd = 2, 128, 4, 64
    drop_p = 0.3
    qkv = (torch.randn(b, s, 3 * nh * hd) * 0.5).bfloat16().cuda() \
        .requires_grad_(True)
    out = _FlashAttention.apply(qkv, None, nh, drop_p, True)
    # recover the mask the forward drew
    ctx_saved = None
    philox = None
    # regenerate via a unit P tensor: entries scaled by 1/keep where kept
    # (dropout_mask_mul_ on ones gives the mask * inv_keep)
    # the philox state is in the autograd ctx; easiest: redo fwd with same
    # generator state is NOT possible (offset advanced) — instead pull the
    # mask from the saved tensors of the graph
    fn = out.grad_fn
    qkv_s, lse_s, philox_s, out_s = fn.saved_tensors
    ones = torch.ones(b * nh, s, s, dtype=torch.bfloat16, device="cuda")
    _hip_ops.dropout_mask_mul_(ones, philox_s, drop_p)
    keep_mask = ones.float()  # inv_keep where kept, 0 where dropped

    gy = torch.randn_like(out)
    out.backward(gy)

    q2 = qkv.detach().float().requires_grad_(True)
    q, k, v = (q2.view(b, s, 3, nh, hd).permute(2, 0, 3, 1, 4)
               .reshape(3, b * nh, s, hd).unbind(0))
    p = torch.softmax((q @ k.transpose(-1, -2)) / hd ** 0.5, dim=-1)
    a = p * keep_mask
    ctx_ref = (a @ v).view(b, nh, s, hd).permute(0, 2, 1, 3).reshape(
        b, s, nh * hd)
    ctx_ref.backward(gy.float())
    diff = (qkv.grad.float() - q2.grad).abs().max().item()
    assert diff < 0.15, diff


def test_fused_adam_device_clip():
    """gscale path == host-side clip + plain adam (reference semantics:
    optimization.py:197 clips before the update)."""
    from oktopk_amd import _hip_ops

    torch.manual_seed(31)
    n = 1_000_033
    for max_norm in (0.5, 1e6):  # firing and non-firing clip
        g = torch.randn(n, device="cuda") * 3.0
        p0 = torch.randn(n, device="cuda")
        # reference: host clip then adam
        gn = g.norm(p=2).item()
        g_ref = g * (max_norm / (gn + 1e-6)) if gn > max_norm else g.clone()
        p_r, m_r, v_r = p0.clone(), torch.zeros_like(g), torch.zeros_like(g)
        _hip_ops.fused_adam_(p_r, g_ref, m_r, v_r, 1e-3, 0.9, 0.999, 1e-6, 0.01)
        # device path
        scale = _hip_ops.grad_clip_scale(g, max_norm)
        assert abs(scale.item() - (max_norm / (gn + 1e-6) if gn > max_norm else 1.0)) < 1e-5
        p_d, m_d, v_d = p0.clone(), torch.zeros_like(g), torch.zeros_like(g)
        _hip_ops.fused_adam_(p_d, g, m_d, v_d, 1e-3, 0.9, 0.999, 1e-6, 0.01,
                             gscale=scale)
        assert torch.allclose(p_d, p_r, atol=1e-6), (p_d - p_r).abs().max()
        assert torch.allclose(m_d, m_r, atol=1e-6)
        # mirror variant
        pb = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
        p_m, m_m, v_m = p0.clone(), torch.zeros_like(g), torch.zeros_like(g)
        _hip_ops.fused_adam_mirror_(p_m, g, m_m, v_m, pb, 1e-3, 0.9, 0.999,
                                    1e-6, 0.01, gscale=scale)
        assert torch.allclose(p_m, p_r, atol=1e-6)
        assert torch.allclose(pb.float(), p_r, atol=0.05, rtol=0.01)


def test_colsum_linear_grads_match_torch():
    """ColsumLinear (kernel bias grad) must match nn.functional.linear's
    autograd on the same bf16 inputs, all three gradients."""
    from oktopk_amd.ops.fused_linear import ColsumLinear

    torch.manual_seed(41)
    for r, c_in, c_out in [(1024, 768, 3072), (7, 768, 768), (64, 64, 2304)]:
        lin = ColsumLinear(c_in, c_out).bfloat16().cuda()
        x = (torch.randn(4, r // 4 if r % 4 == 0 else r, c_in)
             if r % 4 == 0 else torch.randn(1, r, c_in))
        x = x.bfloat16().cuda().requires_grad_(True)
        y = lin(x)
        gy = torch.randn_like(y)
        y.backward(gy)

        x2 = x.detach().clone().requires_grad_(True)
        w2 = lin.weight.detach().clone().requires_grad_(True)
        b2 = lin.bias.detach().clone().requires_grad_(True)
        torch.nn.functional.linear(x2, w2, b2).backward(gy)
        assert torch.allclose(x.grad, x2.grad, atol=1e-2, rtol=1e-2)
        assert torch.allclose(lin.weight.grad, w2.grad, atol=1e-2, rtol=1e-2)
        # bias: fp32-accumulated colsum vs torch's bf16-chain; compare in fp32
        assert torch.allclose(lin.bias.grad.float(), b2.grad.float(),
                              atol=0.05, rtol=0.02), (
            (lin.bias.grad.float() - b2.grad.float()).abs().max())


def test_attn_rowdot_matches_torch():
    from oktopk_amd import _hip_ops

    torch.manual_seed(42)
    b, s, nh, hd = 3, 256, 4, 64
    go = torch.randn(b, s, nh * hd).bfloat16().cuda()
    out = torch.randn(b, s, nh * hd).bfloat16().cuda()
    d = _hip_ops.attn_rowdot(go, out, nh)
    ref = (go.float() * out.float()).view(b, s, nh, hd).sum(-1) \
        .permute(0, 2, 1).reshape(b * nh, s)
    assert torch.allclose(d, ref, atol=1e-2, rtol=1e-3), (d - ref).abs().max()
