"""colsum_bf16_into_exact: the one-launch bias-gradient column sum that adds
in the order of torch's GPU reduction (ops/csrc/direct_grad.hip,
colsum_exact_config.h).  The yardstick is torch itself on the same device,
torch.sum(gy, 0, out=bf16), compared on the raw bits.

Plain randn cannot tell two summation orders apart (the fp32 sums differ far
below one bf16 ulp), so the inputs are cancelling columns: a quarter of the
rows bf16(64*randn), a quarter their negatives, the rest 1e-3*randn, shuffled
independently per column.  test_inputs_discriminate asserts that this data
fails a kernel with another order.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROWS = [1, 7, 63, 64, 65, 300, 515, 1024, 1027, 4096]
COLS = [1, 2, 6, 64, 250, 768, 770, 771, 2304, 3072]
WORKLOAD = [(1024, 768), (1024, 2304), (1024, 3072)]


def hip():
    from oktopk_amd import _hip_ops
    return _hip_ops


def bits(t):
    return t.contiguous().view(torch.int16)


def cancelling(R, C, seed, lead=0):
    """bf16 [R, C] view starting `lead` elements into its allocation.
    Columns 0..2 (where C allows) are all +0.0, all -0.0, and bf16
    subnormals whose sum stays in the subnormal range."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = R // 4
    big = (64 * torch.randn(q, C, device="cuda", generator=g)).bfloat16()
    small = (1e-3 * torch.randn(R - 2 * q, C, device="cuda", generator=g)).bfloat16()
    x = torch.cat([big, -big, small], 0)
    perm = torch.rand(R, C, device="cuda", generator=g).argsort(0)
    x = x.gather(0, perm)
    if C >= 4:
        x[:, 0] = 0.0
        x[:, 1] = -0.0
        x[:, 2] = (torch.randn(R, device="cuda", generator=g) * 2e-40).bfloat16()
    store = torch.empty(R * C + 8, dtype=torch.bfloat16, device="cuda")
    view = store[lead:lead + R * C].view(R, C)
    view.copy_(x)
    return view


def torch_sum(gy):
    out = torch.empty(gy.shape[1], dtype=torch.bfloat16, device="cuda")
    torch.sum(gy, 0, out=out)
    return out


def exact_into(gy, offset, accumulate=False, init=None):
    """Runs the op into a slot `offset` elements into a guarded buffer.
    Returns (supported, slot contents); checks the guard."""
    C = gy.shape[1]
    buf = torch.full((C + 16,), 7.0, dtype=torch.bfloat16, device="cuda")
    slot = buf[offset:offset + C]
    if init is not None:
        slot.copy_(init)
    before = buf.clone()
    ok = hip().colsum_bf16_into_exact(gy, slot, accumulate)
    assert isinstance(ok, bool)
    if not ok:
        assert torch.equal(bits(buf), bits(before)), "unsupported must write nothing"
        return False, None
    assert torch.equal(bits(buf[:offset]), bits(before[:offset])), "bytes before dst"
    assert torch.equal(bits(buf[offset + C:]), bits(before[offset + C:])), "bytes after dst"
    return True, slot.clone()


def check_case(gy, must_support=False):
    R, C = gy.shape
    ref = torch_sum(gy)
    assert torch.isfinite(ref.float()).all()
    ok, got = exact_into(gy, 3)
    if must_support:
        assert ok, f"[{R},{C}] must be supported"
    if not ok:
        return False
    diff = (bits(got) != bits(ref)).sum().item()
    print(f"[{R},{C}] addr%8={gy.data_ptr() % 8}: {diff} of {C} columns differ")
    assert diff == 0
    # accumulate form: reported unsupported, nothing written (torch's
    # bf16 += fp32 add rounds its fp32 operand to bf16 first at some sizes
    # and not at others, see bindings.cpp; the caller keeps torch's calls)
    init = (torch.arange(C, device="cuda") % 13 - 6).bfloat16() * 0.37
    ok2, _ = exact_into(gy, 8, True, init)
    assert not ok2
    return True


@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("R", ROWS)
def test_exact_bits(R, C):
    gy = cancelling(R, C, 1000 * R + C)
    check_case(gy, must_support=(R, C) in WORKLOAD)


@pytest.mark.parametrize("lead", [1, 2])
@pytest.mark.parametrize("R,C", [(1024, 768), (1024, 770), (1027, 771),
                                 (300, 250), (65, 6), (4096, 64)])
def test_exact_bits_offset_source(R, C, lead):
    # torch's vector size drops to 1 / 2 here, and with it the block shape
    gy = cancelling(R, C, 77 * R + C + lead, lead=lead)
    assert gy.data_ptr() % 8 == 2 * lead
    check_case(gy)


def test_exact_bits_vocab():
    check_case(cancelling(1024, 30522, 5))


def test_workload_config():
    """The configuration the port derives for the three workload shapes on
    this device, and that they run the kernel."""
    p = torch.cuda.get_device_properties(0)
    for R, C in WORKLOAD:
        gy = cancelling(R, C, 3)
        cfg = hip().colsum_exact_config(R, C, gy.data_ptr(), p.multi_processor_count,
                                        p.max_threads_per_multi_processor, p.warp_size)
        print(f"[{R},{C}] (V, bw, bh, split, ctas) = {cfg}")
        assert cfg is not None
        ok, _ = exact_into(gy, 5)
        assert ok
    # outside the family
    assert hip().colsum_exact_config(1, 64, 0, 256, 2048, 64) is None
    assert hip().colsum_exact_config(64, 1, 0, 256, 2048, 64) is None
    assert hip().colsum_exact_config(1 << 20, 1 << 12, 0, 256, 2048, 64) is None
    t = torch.zeros(8, 16, dtype=torch.bfloat16, device="cuda")[:, ::2]
    dst = torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    assert hip().colsum_bf16_into_exact(t, dst, False) is False


def test_inputs_discriminate():
    """The old one-launch kernel (its own order) must differ from torch on
    this data: proof that the data can fail a wrong order."""
    gy = cancelling(1024, 768, 1000 * 1024 + 768)
    ref = torch_sum(gy)
    old = torch.empty_like(ref)
    hip().colsum_bf16_into(gy, old, False)
    ndiff = (bits(old) != bits(ref)).sum().item()
    print(f"colsum_bf16_into vs torch: {ndiff} of 768 columns differ")
    assert ndiff >= 1


def test_run_to_run():
    gy = cancelling(1024, 3072, 11)
    ok, a = exact_into(gy, 3)
    assert ok
    for _ in range(2):
        _, b = exact_into(gy, 3)
        assert torch.equal(bits(a), bits(b))


def test_nonfinite_columns_keep_their_class():
    gy = cancelling(1024, 768, 12)
    gy[5, 10] = float("nan")
    gy[6, 11] = float("inf")
    gy[7, 12] = float("-inf")
    gy[8, 13] = float("inf")
    gy[9, 13] = float("-inf")          # inf - inf -> nan
    gy[:, 14] = 3.0e38                 # overflows to inf in fp32
    ref = torch_sum(gy).float()
    ok, got = exact_into(gy, 3)
    assert ok
    got = got.float()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(torch.isposinf(got), torch.isposinf(ref))
    assert torch.equal(torch.isneginf(got), torch.isneginf(ref))
    fin = torch.isfinite(ref)
    assert torch.equal(bits(got.bfloat16()[fin]), bits(ref.bfloat16()[fin]))
    assert torch.isnan(ref[10]) and torch.isposinf(ref[11]) and torch.isneginf(ref[12])


@pytest.mark.parametrize("N", [768, 30522])
def test_linear_bwd_into_accumulate_keeps_torch_bits(N):
    """Accumulating into a slot with bias_exact set: the bits of torch's
    slot.add_(sum(gy, 0, dtype=fp32)), at a size on either side of the
    switch in torch's mixed-dtype add."""
    g = torch.Generator(device="cuda").manual_seed(6)
    gy = cancelling(1024, N, 31)
    x = torch.randn(1024, 8, device="cuda", generator=g).bfloat16()
    w = torch.randn(N, 8, device="cuda", generator=g).bfloat16()
    init = ((torch.arange(N, device="cuda") % 13 - 6) * 0.37).bfloat16()
    ref = init.clone().add_(torch.sum(gy, 0, dtype=torch.float32))
    gb = init.clone()
    hip().linear_bwd_into(gy, x, w, None, gb, True, False, True)
    assert torch.equal(bits(gb), bits(ref))


def test_linear_bwd_into_trailing_argument():
    """bias_exact as the optional trailing argument: torch's bits in the
    slot; the positional (accumulate, bias_kernel) call keeps its meaning."""
    g = torch.Generator(device="cuda").manual_seed(4)
    gy = cancelling(1024, 768, 21)
    x = torch.randn(1024, 64, device="cuda", generator=g).bfloat16()
    w = torch.randn(768, 64, device="cuda", generator=g).bfloat16()
    ref = torch_sum(gy)
    slots = []
    for args in ((False, False, True), (False, False), (False, True)):
        gb = torch.full((768,), 7.0, dtype=torch.bfloat16, device="cuda")
        hip().linear_bwd_into(gy, x, w, None, gb, *args)
        slots.append(gb)
    assert torch.equal(bits(slots[0]), bits(ref))
    assert torch.equal(bits(slots[1]), bits(ref))
    old = torch.empty_like(ref)
    hip().colsum_bf16_into(gy, old, False)
    assert torch.equal(bits(slots[2]), bits(old))


SMALL = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2,
             intermediate_size=256, vocab_size=1000,
             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _bert_grads(monkeypatch, colsum_bias):
    from oktopk_amd.config import EngineConfig, OkTopkConfig
    from oktopk_amd.ops.fused_linear import bias_grad_mode
    from oktopk_amd.trainer import Trainer

    if colsum_bias is None:
        monkeypatch.delenv("OKTOPK_COLSUM_BIAS", raising=False)
        assert bias_grad_mode() == "exact"
    else:
        monkeypatch.setenv("OKTOPK_COLSUM_BIAS", colsum_bias)
        assert bias_grad_mode() == "torch"
    monkeypatch.setenv("OKTOPK_DIRECT_GRAD", "1")
    torch.manual_seed(0)
    cfg = EngineConfig(compressor="oktopk", density=0.01,
                       oktopk=OkTopkConfig(dense_warmup_iters=0))
    tr = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg,
                 model_kwargs=SMALL, dtype="bf16")
    tr.batches.input_ids.clamp_(max=999)
    tr.batches.mlm_labels.clamp_(max=999)
    assert tr.opt._dg_owner is not None
    b, model = tr.batches, tr.model
    tr.opt.zero_grad()
    tr.opt.set_substep(0)
    logits, nsp_logits = model(b.input_ids, token_type_ids=b.token_type,
                               attention_mask=b.attn)
    loss = F.cross_entropy(logits.view(-1, logits.size(-1)),
                           b.mlm_labels.view(-1), ignore_index=-1)
    loss = loss + F.cross_entropy(nsp_logits.view(-1, 2), b.nsp.view(-1))
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.clone() for n, p in model.named_parameters()}


def test_bert_grads_equal_torch_reduction(monkeypatch):
    """Small bf16 BERT, every parameter gradient: default (exact kernel) vs
    OKTOPK_COLSUM_BIAS=0 (torch's reduction)."""
    ref = _bert_grads(monkeypatch, "0")
    got = _bert_grads(monkeypatch, None)
    assert set(ref) == set(got)
    for name, r in ref.items():
        assert torch.equal(bits(got[name]), bits(r)), name
