"""The fused CTC loss kernel (ops/csrc/ctc_loss.hip) against ctc_loss_ref in
fp64 on the CPU.  Yardstick: ctc_loss_ref in fp32 on the CPU on the same
inputs.  Gradient: rel_fro(kernel) <= CTC_REF32_FACTOR * rel_fro(yardstick);
loss: rel error <= CTC_REF32_FACTOR * max(yardstick's, CTC_LOSS_FLOOR); rows
past an input length exactly 0.  reduction="none" with utterance n weighted
n + 1 in the backward; logits standard normal, labels uniform over the
non-blank classes, the first two labels of a target equal where every input length
is at least 2 L.
Measured ratios: profiles/README.md r19.
"""
import functools

import pytest
import torch

from oktopk_amd.ops import reference as R
from oktopk_amd.ops.hip_ctc import ctc_loss, hip_ctc_available

pytestmark = pytest.mark.gpu


def build(T, N, C, L, blank=0, in_lens=None):
    """fp64 CPU (logits, padded targets, input lengths, target lengths)."""
    g = torch.Generator().manual_seed(T * 1000 + L + 2)
    logits = torch.randn(T, N, C, generator=g, dtype=torch.float64)
    r = torch.randint(0, C - 1, (N, L), generator=g)
    targets = r + (r >= blank)
    if L >= 2 and min(in_lens or [T]) >= 2 * L:  # room for every repeat's blank
        targets[:, 1] = targets[:, 0]
    in_len = torch.tensor(in_lens or [T] * N, dtype=torch.int32)
    return logits, targets, in_len, torch.full((N,), L, dtype=torch.int32)


def run(fn, logits, *rest, reduction="none", **kw):
    """(loss, gradient at the logits) of fn, utterance n weighted n + 1."""
    x = logits.detach().requires_grad_()
    loss = fn(x, *rest, reduction=reduction, **kw)
    w = torch.arange(1, x.size(1) + 1, device=x.device, dtype=x.dtype)
    (grad,) = torch.autograd.grad((loss * w).sum() if reduction == "none" else loss, x)
    return loss.detach(), grad


@functools.lru_cache(maxsize=None)
def cpu_side(shape, blank=0, in_lens=None, reduction="none", zero_infinity=False):
    """(fp64 inputs, fp64 oracle, the fp32 yardstick's (loss, gradient))."""
    inputs = build(*shape, blank=blank, in_lens=in_lens)
    kw = dict(blank=blank, reduction=reduction, zero_infinity=zero_infinity)
    ref64 = run(R.ctc_loss_ref, *inputs, **kw)
    ref32 = run(R.ctc_loss_ref, inputs[0].float(), *inputs[1:], **kw)
    return inputs, ref64, ref32


def on_gpu(inputs):
    return [inputs[0].float().cuda()] + [a.cuda() for a in inputs[1:]]


def check(got, ref64, ref32, in_len, utts=None):
    """The rule of the module docstring over the utterances `utts` (all)."""
    utts = list(utts if utts is not None else range(len(in_len)))
    (loss, grad), (loss64, grad64), (loss32, grad32) = [
        (l.reshape(-1).cpu()[utts if l.dim() else [0]], g.cpu()[:, utts])
        for l, g in (got, ref64, ref32)]
    for i, n in enumerate(utts):
        assert not grad[int(in_len[n]):, i].any(), "gradient past the input length"
    assert torch.isfinite(loss64).all()
    err, yard = R.lstm_rel_fro(grad, grad64), R.lstm_rel_fro(grad32, grad64)
    lerr, lyard = R.lstm_rel_fro(loss, loss64), R.lstm_rel_fro(loss32, loss64)
    print(f"grad: kernel {err:.3e} yardstick {yard:.3e} ratio {err / yard:.2f}; "
          f"loss: kernel {lerr:.3e} yardstick {lyard:.3e}")
    assert err <= R.CTC_REF32_FACTOR * yard
    assert lerr <= R.CTC_REF32_FACTOR * max(lyard, R.CTC_LOSS_FLOOR)


# (T, N, C, L): see profiles/README.md r19 for what each shape exercises;
# (182, 2, 29, 20) is the largest T whose lattices stay in LDS at L = 20.
@pytest.mark.parametrize("shape, kw", [
    ((1, 1, 2, 0), {}), ((1, 1, 2, 1), {}), ((2, 3, 29, 1), {}),
    ((7, 3, 29, 3), {}), ((70, 2, 29, 31), {}), ((70, 2, 29, 32), {}),
    ((140, 2, 70, 64), {}), ((300, 2, 29, 127), {}), ((182, 2, 29, 20), {}),
    ((183, 2, 29, 20), {}),
    ((7, 3, 29, 3), dict(in_lens=(7, 4, 6))),
    ((7, 3, 29, 3), dict(blank=28)),
    ((7, 3, 29, 3), dict(reduction="mean")),
    ((7, 3, 29, 3), dict(reduction="sum")),
])
def test_against_fp64(shape, kw):
    inputs, ref64, ref32 = cpu_side(shape, **kw)
    gpu = on_gpu(inputs)
    assert hip_ctc_available(*gpu)
    kw = {k: v for k, v in kw.items() if k != "in_lens"}  # in the inputs already
    check(run(ctc_loss, *gpu, **kw), ref64, ref32, inputs[2])


@pytest.mark.parametrize("zero_infinity", [True, False])
def test_infeasible_utterance(zero_infinity):
    inputs, ref64, ref32 = cpu_side((4, 2, 5, 3), in_lens=(2, 4),
                                    zero_infinity=zero_infinity)
    loss, grad = run(ctc_loss, *on_gpu(inputs), zero_infinity=zero_infinity)
    if zero_infinity:
        assert loss[0] == 0 and not grad[:, 0].any()
    else:
        assert loss[0] == float("inf")
    check((loss, grad), ref64, ref32, inputs[2], utts=[1])


def test_layouts_and_length_dtypes_agree_to_the_bit():
    logits, targets, in_len, _ = on_gpu(build(40, 3, 9, 10))
    tgt_len = torch.tensor([10, 4, 7], dtype=torch.int32).cuda()
    padded = run(ctc_loss, logits, targets, in_len, tgt_len)
    flat = torch.cat([targets[n, :l] for n, l in enumerate(tgt_len.tolist())])
    for other in (run(ctc_loss, logits, flat, in_len, tgt_len),
                  run(ctc_loss, logits, flat.int(), in_len.long(), tgt_len.long())):
        assert all(torch.equal(a, b) for a, b in zip(padded, other))


def test_graph_replays_equal_eager():
    gpu = on_gpu(build(70, 3, 29, 32, in_lens=(70, 50, 66)))
    eager = run(ctc_loss, *gpu)
    assert all(torch.equal(a, b) for a, b in zip(run(ctc_loss, *gpu), eager))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(ctc_loss, *gpu)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(ctc_loss, *gpu)
    for _ in range(3):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_trainer_captures_lstman4(monkeypatch):
    from oktopk_amd.comm import Comm
    from oktopk_amd.trainer import Trainer

    monkeypatch.setenv("OKTOPK_HIP_LSTM", "1")
    monkeypatch.setenv("OKTOPK_HIP_CTC", "1")
    tr = Trainer(model_name="lstman4", batch_size=2, comm=Comm(None), dtype="fp32")
    assert tr.capture_graph()
    tr.opt.zero_grad()
    tr._graph.replay()
    replayed = tr._graph_loss.detach().double().cpu()
    eager = tr._forward_loss().detach().double().cpu()
    assert torch.isfinite(replayed)
    assert abs(replayed - eager) <= R.CTC_REF32_FACTOR * R.CTC_LOSS_FLOOR * abs(eager)
