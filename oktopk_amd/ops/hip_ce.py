"""Cross-entropy of raw logits on hand-written HIP kernels
(ops/csrc/cross_entropy.hip): forward keeps the row maximum and the log of
the row's sum of exponentials, backward recomputes the softmax from them and
writes the gradient in one pass.  No log-probability tensor is made, rows that
carry `ignore_index` read no logits, and targets are read on the device, so
the loss is capturable in a graph.

The callers (models/bert.py, `Trainer._forward_loss`, pipeline.py) go through
`cross_entropy`.  It takes the kernels when OKTOPK_HIP_CE=1 and
`hip_ce_available` holds; otherwise it calls F.cross_entropy with the caller's
own arguments (profiles/README.md r20 has the A/B).

On the kernel path the loss is fp32 whatever the logits' dtype; the gradient
is in the logits' dtype.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

_INT = (torch.int32, torch.int64)
_FLOAT = (torch.float32, torch.bfloat16)
_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def hip_ce_enabled() -> bool:
    return os.environ.get("OKTOPK_HIP_CE", "0") == "1"


def hip_ce_available(logits, target) -> bool:
    """Whether the kernels take the case, from shapes and dtypes alone: fp32 or
    bf16 contiguous logits [R, C] on the GPU with R, C >= 1 and under 2^31
    bytes, int32 / int64 class targets [R] on the same device, with the
    extension built.  (Under autocast F.cross_entropy upcasts bf16 logits to
    fp32 first; the kernels read them as they are, which is the same values.)"""
    if not (logits.is_cuda and logits.dim() == 2 and logits.dtype in _FLOAT
            and logits.is_contiguous() and min(logits.shape) >= 1
            and logits.numel() * logits.element_size() < 2 ** 31):
        return False
    if (target.dtype not in _INT or target.device != logits.device
            or target.shape != (logits.size(0),)):
        return False
    from . import hip_available

    return hip_available()


class _CrossEntropyFn(torch.autograd.Function):
    """loss (fp32: [R] or 0-dim); saves (logits, target, stats, factor)."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, reduction):
        from . import _backend

        target = target.contiguous()
        loss, stats, factor = _backend(logits).ce_fwd(
            logits, target, ignore_index, reduction)
        ctx.save_for_backward(logits, target, stats, factor)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        from . import _backend

        logits, target, stats, factor = ctx.saved_tensors
        grad = _backend(logits).ce_bwd(
            logits, target, stats, factor,
            g_loss.float().contiguous().view(-1), ctx.ignore_index)
        return grad, None, None, None


def cross_entropy(logits, target, ignore_index: int = -100,
                  reduction: str = "mean"):
    """F.cross_entropy(logits, target, ignore_index=..., reduction=...) for
    class-index targets.  On the kernel path: an ignored row has loss 0 and a
    zero gradient row; 'mean' divides by the number of rows that are not
    ignored (NaN when there is none); a label outside [0, C) that is not
    `ignore_index` gives that row a NaN loss and a zero gradient row.
    Differentiable in logits."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"cross_entropy: unknown reduction {reduction!r}")
    if not (hip_ce_enabled() and hip_ce_available(logits, target)):
        return F.cross_entropy(logits, target, ignore_index=ignore_index,
                               reduction=reduction)
    return _CrossEntropyFn.apply(logits, target, int(ignore_index),
                                 _REDUCTIONS[reduction])
