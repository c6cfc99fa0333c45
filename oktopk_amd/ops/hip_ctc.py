"""CTC loss from raw logits on a hand-written HIP kernel
(ops/csrc/ctc_loss.hip): one launch computes the negative log-likelihood of
every utterance and, when a gradient is wanted, the gradient at the raw
logits; the log-softmax is fused in.  Lengths and targets are read on the
device and nothing is staged through the host, so the loss can be captured
in a graph — which torch's GPU ctc_loss, with its host-side lengths, cannot.

`Trainer._forward_loss` takes this path for lstman4 when OKTOPK_HIP_CTC=1 and
`hip_ctc_available` holds; otherwise it calls F.log_softmax + F.ctc_loss as
before (profiles/README.md r19 has the A/B).  On a CPU tensor, or when the
kernel does not take the case, `ctc_loss` runs `reference.ctc_loss_ref`.

Target lengths: padded targets [N, Lmax] need Lmax <= 127.  For 1-D
concatenated targets the longest length is not known without a sync; the
kernel is then launched for up to 127 and reports an utterance whose target
is longer (or, padded, longer than Lmax) as NaN loss with a zero gradient.
"""
from __future__ import annotations

import os

import torch

from . import reference as _ref

_INT = (torch.int32, torch.int64)
MAX_TARGET_LENGTH = 127


def hip_ctc_enabled() -> bool:
    return os.environ.get("OKTOPK_HIP_CTC", "0") == "1"


def hip_ctc_available(logits, targets, input_lengths, target_lengths) -> bool:
    """Whether the kernel takes the case, from shapes and dtypes alone: fp32
    contiguous logits [T, N, C] on the GPU with T, N, C >= 1, int32 / int64
    lengths [N] and targets ([N, Lmax <= 127] or 1-D) on the same device,
    outside autocast, with the extension built."""
    if not (logits.is_cuda and logits.dim() == 3
            and logits.dtype == torch.float32 and logits.is_contiguous()
            and min(logits.shape) >= 1 and not torch.is_autocast_enabled()):
        return False
    n = logits.size(1)
    for t in (targets, input_lengths, target_lengths):
        if t.dtype not in _INT or t.device != logits.device:
            return False
    if input_lengths.shape != (n,) or target_lengths.shape != (n,):
        return False
    if targets.dim() == 2:
        if targets.size(0) != n or targets.size(1) > MAX_TARGET_LENGTH:
            return False
    elif targets.dim() != 1:
        return False
    from . import hip_available

    return hip_available()


class _CtcLossFn(torch.autograd.Function):
    """nll [N]; the gradient at the logits is made in forward and saved."""

    @staticmethod
    def forward(ctx, logits, targets, input_lengths, target_lengths, blank,
                zero_infinity):
        from . import _backend

        want_grad = ctx.needs_input_grad[0]
        nll, grad = _backend(logits).ctc_loss_fwd(
            logits, targets.contiguous(), input_lengths.contiguous(),
            target_lengths.contiguous(), blank, zero_infinity, want_grad)
        if want_grad:
            ctx.save_for_backward(grad)
        return nll

    @staticmethod
    def backward(ctx, g_nll):
        from . import _backend

        (grad,) = ctx.saved_tensors
        out = _backend(grad).ctc_scale_grad(grad, g_nll.float().contiguous())
        return out, None, None, None, None, None


def ctc_loss(logits, targets, input_lengths, target_lengths, blank: int = 0,
             reduction: str = "mean", zero_infinity: bool = False):
    """CTC loss of raw logits [T, N, C]: F.ctc_loss(F.log_softmax(logits, -1),
    ...) with torch's reductions ('mean' divides each loss by
    clamp(target_length, 1), then averages; 'sum'; 'none').  targets: padded
    [N, Lmax] or 1-D concatenated; input lengths are clamped to T; a label
    outside [0, C) makes its utterance impossible.  An infeasible utterance
    has loss +inf and an unspecified gradient, or loss 0 and gradient 0 with
    zero_infinity.  Differentiable in logits."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"ctc_loss: unknown reduction {reduction!r}")
    if not hip_ctc_available(logits, targets, input_lengths, target_lengths):
        return _ref.ctc_loss_ref(logits, targets, input_lengths, target_lengths,
                                 blank, reduction, zero_infinity)
    if not 0 <= int(blank) < logits.size(2):
        raise ValueError("ctc_loss: blank must be in [0, C)")
    nll = _CtcLossFn.apply(logits, targets, input_lengths, target_lengths,
                           int(blank), bool(zero_infinity))
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    return (nll / target_lengths.clamp(min=1).to(nll.dtype)).mean()
