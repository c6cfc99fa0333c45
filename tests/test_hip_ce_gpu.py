"""The fused cross-entropy kernels (ops/csrc/cross_entropy.hip) against
cross_entropy_ref in fp64 on the CPU.  Yardstick: the same function in fp32 on
the CPU on the same inputs; for bf16 the inputs are bf16 values upcast exactly
and the yardstick's gradient is rounded to bf16 once.  Gradient:
rel_fro(kernel) <= CE_REF32_FACTOR * rel_fro(yardstick); loss: rel error <=
CE_REF32_FACTOR * max(yardstick's, CE_LOSS_FLOOR); ignored rows exactly 0.
reduction="none" with row r weighted r + 1 in the backward.  Logits standard
normal; row 1 scaled by 50 (a missing max subtraction overflows there), row 2
with -inf entries away from its label.  Measured ratios: profiles/README.md r20.
"""
import functools

import pytest
import torch

from oktopk_amd._hip_ops import ce_fwd  # noqa: F401  (the kernels must be built)
from oktopk_amd.ops import reference as R
from oktopk_amd.ops.hip_ce import cross_entropy, hip_ce_available

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    monkeypatch.setenv("OKTOPK_HIP_CE", "1")


def build(rows, C, dtype, place, ignore_index=-100):
    """fp64 CPU (logits holding `dtype` values exactly, int64 targets).  The
    first row is ignored, from 5 rows on the last one too.  The labelled rows
    take their labels from (0, C - 1, 1: inside the head peel of a row that
    starts off a 16-byte boundary, C - 2: inside the tail), starting at
    2 * place."""
    g = torch.Generator().manual_seed(rows * 100003 + C)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64)
    x[1] *= 50
    spots = (0, C - 1, min(1, C - 1), max(C - 2, 0))
    target = torch.tensor([spots[(r - 1 + 2 * place) % 4] for r in range(rows)])
    target[0] = ignore_index
    if rows >= 5:
        target[-1] = ignore_index
    for d in (1, 3, C // 2):
        if (int(target[2]) + d) % C != int(target[2]):
            x[2, (int(target[2]) + d) % C] = float("-inf")
    return x.to(dtype).double(), target


def run(fn, x, target, reduction="none", **kw):
    """(loss, gradient at the logits) of fn, row r weighted r + 1."""
    x = x.detach().requires_grad_()
    loss = fn(x, target, reduction=reduction, **kw)
    w = torch.arange(1, x.size(0) + 1, device=x.device, dtype=loss.dtype)
    (grad,) = torch.autograd.grad((loss * w).sum() if reduction == "none" else loss, x)
    return loss.detach(), grad


@functools.lru_cache(maxsize=None)
def cpu_side(rows, C, dtype, place, reduction="none", ignore_index=-100):
    """(fp64 inputs, fp64 oracle, the fp32 yardstick's (loss, gradient))."""
    x, target = build(rows, C, dtype, place, ignore_index)
    kw = dict(reduction=reduction, ignore_index=ignore_index)
    ref64 = run(R.cross_entropy_ref, x, target, **kw)
    loss32, grad32 = run(R.cross_entropy_ref, x.float(), target, **kw)
    return (x, target), ref64, (loss32, grad32.to(dtype))


def rel(x, ref64):
    """lstm_rel_fro; against an all-zero reference (C = 1) 0 if x is all zero."""
    if ref64.any():
        return R.lstm_rel_fro(x, ref64)
    return float("inf") if x.any() else 0.0


def check(got, ref64, ref32, target, ignore_index=-100):
    (loss, grad), (loss64, grad64), (loss32, grad32) = got, ref64, ref32
    assert loss.dtype == F32 and torch.isfinite(loss64).all()
    assert not grad[(target == ignore_index).to(grad.device)].any(), "ignored row"
    err, yard = rel(grad, grad64), rel(grad32, grad64)
    lerr, lyard = rel(loss, loss64), rel(loss32, loss64)
    print(f"grad: kernel {err:.3e} yardstick {yard:.3e}; "
          f"loss: kernel {lerr:.3e} yardstick {lyard:.3e}")
    assert err <= R.CE_REF32_FACTOR * yard
    assert lerr <= R.CE_REF32_FACTOR * max(lyard, R.CE_LOSS_FLOOR)


# C <= 1024: a wave per row; above: a block per row.  63 / 65 and 1024 / 1025
# / 2051 sit around the vector width and that threshold; odd C leaves rows
# 2-byte (bf16) or 4-byte (fp32) aligned.
CASES = [((5, C, dt, place), {}) for C in (1, 2, 7, 8, 9, 63, 65, 1024, 1025, 2051)
         for dt in (F32, BF16) for place in (0, 1)]
CASES += [((3, 30522, BF16, place), dict(ignore_index=-1)) for place in (0, 1)]
CASES += [((3, 10000, F32, place), {}) for place in (0, 1)]
CASES += [((5, 65, dt, 0), dict(offset=1)) for dt in (F32, BF16)]
CASES += [((5, C, dt, 1), dict(reduction=red)) for C in (9, 2051)
          for dt in (F32, BF16) for red in ("mean", "sum")]


@pytest.mark.parametrize("shape, kw", CASES)
def test_against_fp64(shape, kw):
    kw = dict(kw)
    offset = kw.pop("offset", 0)  # the view starts `offset` elements into its storage
    (x, target), ref64, ref32 = cpu_side(*shape, **kw)
    buf = torch.empty(x.numel() + offset, dtype=shape[2], device="cuda")
    xg = buf[offset:].view_as(x).copy_(x)
    assert xg.storage_offset() == offset and hip_ce_available(xg, target.cuda())
    got = run(cross_entropy, xg, target.cuda(), **kw)
    assert got[1].dtype == shape[2]
    check(got, ref64, ref32, target, kw.get("ignore_index", -100))


def test_target_dtypes_agree_to_the_bit():
    x, target = build(5, 2051, BF16, 0)
    x, target = x.bfloat16().cuda(), target.cuda()
    a, b = run(cross_entropy, x, target), run(cross_entropy, x, target.int())
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("C", [9, 2051])
def test_all_rows_ignored(C):
    x = torch.randn(5, C, device="cuda")
    target = torch.full((5,), -100, device="cuda")
    loss, grad = run(cross_entropy, x, target, reduction="mean")
    assert torch.isnan(loss) and not grad.any()
    loss, grad = run(cross_entropy, x, target, reduction="sum")
    assert loss == 0 and not grad.any()


@pytest.mark.parametrize("C, bad", [(9, 9), (9, -5), (2051, 1 << 40)])
def test_label_out_of_range(C, bad):
    x, target = build(5, C, F32, 0)
    target[2] = bad
    loss, grad = run(cross_entropy, x.float().cuda(), target.cuda())
    assert torch.isnan(loss[2]) and torch.isfinite(loss[[0, 1, 3, 4]]).all()
    assert not grad[2].any() and grad[1].any() and torch.isfinite(grad).all()


def test_graph_replays_equal_eager():
    x, target = build(5, 2051, BF16, 1)
    x, target = x.bfloat16().cuda(), target.cuda()
    both = lambda: (*run(cross_entropy, x, target, reduction="mean"),
                    *run(cross_entropy, x[:, :65].contiguous(), target % 65))
    eager = both()
    assert all(torch.equal(a, b) for a, b in zip(both(), eager))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = both()
    for _ in range(3):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_bert_loss_and_gradients(monkeypatch):
    """BertForPreTraining (2 layers, hidden 128, vocab 2051, b = 2, s = 128,
    bf16, no dropout): loss and every parameter gradient, rounded to bf16, with
    the switch set against the switch unset.  The unset arm takes its loss from
    log-probabilities rounded to bf16; how far that rounding alone moves the
    result is measured by a third arm, unset with the logits upcast to fp32
    before F.cross_entropy.  Bound: 3 times that distance (loss: relative;
    gradients: the largest rel_fro over the parameters, since the loss reaches
    every parameter through the one logits gradient).
    Measured on an MI355X at the commit that added this test: the bf16 losses
    of all three arms are equal (distance 0, bound 0); gradients upcast/unset
    3.458e-2 (bound 1.04e-1), set/unset 3.458e-2."""
    import torch.nn.functional as F

    from oktopk_amd.config import EngineConfig, OkTopkConfig
    from oktopk_amd.trainer import Trainer

    torch.manual_seed(0)
    cfg = EngineConfig(compressor="oktopk", density=0.01,
                       oktopk=OkTopkConfig(dense_warmup_iters=0))
    small = dict(num_hidden_layers=2, hidden_size=128, num_attention_heads=2,
                 intermediate_size=256, vocab_size=2051, hidden_dropout_prob=0.0,
                 attention_probs_dropout_prob=0.0)
    tr = Trainer("bert_base", batch_size=2, seq_len=128, cfg=cfg, model_kwargs=small,
                 dtype="bf16")
    tr.batches.input_ids.clamp_(max=2050)
    tr.batches.mlm_labels.clamp_(max=2050)
    assert (tr.batches.mlm_labels >= 0).any() and (tr.batches.mlm_labels == -1).any()

    def arm():
        tr.opt.zero_grad()
        tr.opt.set_substep(0)
        loss = tr._forward_loss()
        loss.backward()
        return [loss.detach().bfloat16().double()] + [
            p.grad.bfloat16().double() for p in tr.model.parameters()]

    def distance(a, b):
        rel = [float((x - y).norm() / y.norm()) for x, y in zip(a, b)]
        return rel[0], max(rel[1:])

    on = arm()
    monkeypatch.delenv("OKTOPK_HIP_CE")
    off = arm()
    plain = F.cross_entropy
    monkeypatch.setattr(F, "cross_entropy",
                        lambda x, *a, **kw: plain(x.float(), *a, **kw))
    upcast = arm()
    (lgot, ggot), (lbound, gbound) = distance(on, off), distance(upcast, off)
    print(f"loss: set/unset {lgot:.3e} upcast/unset {lbound:.3e}; "
          f"grad: set/unset {ggot:.3e} upcast/unset {gbound:.3e}")
    assert torch.isfinite(off[0]) and gbound > 0
    assert lgot <= 3 * lbound and ggot <= 3 * gbound
