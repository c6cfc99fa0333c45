"""y = LayerNorm(x + dropout(a)) with one kernel of ours each way, bit for bit
what torch's kernels compute (ops/csrc/residual_ln.hip).

Forward: torch's own native_dropout (mask and RNG stream untouched), then one
launch for the residual add, the row moments and the normalisation, in place
of torch's add, RowwiseMomentsCUDAKernel and LayerNormForwardCUDAKernel.
Backward: one launch for the LayerNorm input gradient and the dropout
backward, in place of layer_norm_grad_input_kernel and masked_scale_kernel;
the gamma / beta gradients are those of torch's native_layer_norm_backward,
computed by the batched launch at the end of the pass that leaves the same
bits (by torch itself with OKTOPK_BATCH_LN_GRADS=0 or an unsupported row
count), and go to the deferred add slots exactly as in slot_ln.py.

A site's output feeds the next sub-layer's GEMM and the next residual add, and
autograd would add the two incoming gradients with a kernel of its own.  The
Function therefore returns two tensors over one storage: y for the GEMM and,
as y's `_residual_edge` attribute, the same values for the next residual add
(residual_edge() looks it up; a tensor without it, as across a pipeline
stage boundary, is its own edge).  Backward then receives the two gradients
apart and the kernel adds them; where only one arrives it takes that one.

On by default; OKTOPK_FUSED_RESIDUAL_LN=0 restores the unfused path (read at
each call; profiles/README.md r15 has the A/B).  Not taken with
OKTOPK_DIRECT_LN=1, nor where torch itself would run
another kernel: its vectorised LayerNorm forward, which sums in another order,
is what torch launches when x, gamma and beta are all 8-byte aligned, so the
fused path needs gamma or beta off that alignment.  That hinges on the layout
of the flat parameter buffer: in the flagship the 30522-element decoder bias
leads its group and shifts every LayerNorm parameter 4 bytes off; with a
vocabulary padded to a multiple of 4, or another parameter order, every site
takes the unfused path (tests/test_residual_ln_gpu.py checks the flagship's
sites).  Reproducing the vectorised kernel's order is future work.
Everything else takes the unfused path.
"""
from __future__ import annotations

import os

import torch

from .fused_linear import _ADD_SLOT_ATTR
from .slot_ln import defer_ln_param_grad_sums, defer_ln_param_grads


def residual_ln_enabled() -> bool:
    env = os.environ
    return (env.get("OKTOPK_FUSED_RESIDUAL_LN", "1") != "0"
            and env.get("OKTOPK_DIRECT_LN", "0") != "1")


def torch_takes_rowwise_ln(x, w, b) -> bool:
    """Whether native_layer_norm runs RowwiseMoments + LayerNormForward for
    these bf16 tensors (else: its vectorised kernel)."""
    return bool((x.data_ptr() | w.data_ptr() | b.data_ptr()) & 7) or x.shape[-1] % 4 != 0


def residual_ln_available(x, a, ln) -> bool:
    if not (residual_ln_enabled() and x.is_cuda and torch.is_grad_enabled()
            and x.dtype == torch.bfloat16 and a.dtype == torch.bfloat16
            and x.shape == a.shape and ln.training
            and isinstance(ln, torch.nn.LayerNorm) and ln.elementwise_affine
            and ln.bias is not None and len(ln.normalized_shape) == 1
            and ln.weight.dtype == torch.bfloat16
            and ln.weight.is_contiguous() and ln.bias.is_contiguous()
            and hasattr(ln.weight, _ADD_SLOT_ATTR) and hasattr(ln.bias, _ADD_SLOT_ATTR)):
        return False
    from . import hip_available

    if not hip_available():
        return False
    from oktopk_amd import _hip_ops

    return (_hip_ops.residual_ln_supported(x.shape[-1])
            and x.is_contiguous() and a.is_contiguous()
            and x.data_ptr() % 8 == 0 and a.data_ptr() % 8 == 0
            and torch_takes_rowwise_ln(x, ln.weight, ln.bias))


class _ResidualLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, w, b, eps, p, train):
        from oktopk_amd import _hip_ops

        mask = None
        d = a
        if train and p > 0.0:
            d, mask = torch.native_dropout(a, p, True)
        y, s, mean, rstd = _hip_ops.residual_ln_fwd(x, d, w, b, eps)
        ctx.save_for_backward(s, mean, rstd, w, b, mask)
        # native_dropout_backward's scale (derivatives.yaml)
        ctx.scale = 0.0 if p == 1 else 1.0 / (1.0 - p)
        ctx.set_materialize_grads(False)
        # the view first: it can carry the base as an attribute without a
        # reference cycle
        return y.view_as(y), y

    @staticmethod
    def backward(ctx, gy1, gy2):
        from oktopk_amd import _hip_ops

        s, mean, rstd, w, b, mask = ctx.saved_tensors
        need = ctx.needs_input_grad
        H = s.shape[-1]
        if gy1 is None:
            gy1, gy2 = gy2, None
        if gy1 is None:
            return (None,) * 7
        gy1 = _aligned(gy1)
        if gy2 is not None:
            gy2 = _aligned(gy2)
        gy, gs, ga = _hip_ops.residual_ln_bwd(gy1, gy2, s, mean, rstd, w, mask,
                                              ctx.scale)
        gw = gb = None
        if need[2] and need[3] and defer_ln_param_grad_sums(w, b, gy, s, mean, rstd):
            pass
        elif need[2] or need[3]:
            stat_shape = s.shape[:-1] + (1,)
            _, gw, gb = torch.ops.aten.native_layer_norm_backward(
                gy, s, [H], mean.view(stat_shape), rstd.view(stat_shape), w, b,
                [False, bool(need[2]), bool(need[3])])
            if need[2] and need[3] and defer_ln_param_grads(w, b, gw, gb):
                gw = gb = None
        return (gs if need[0] else None, ga if need[1] else None, gw, gb,
                None, None, None)


def _aligned(g):
    g = g.contiguous()
    return g.clone() if g.data_ptr() % 8 else g


_EDGE_ATTR = "_residual_edge"


def residual_edge(x):
    """The tensor the next residual add should read in place of x."""
    return getattr(x, _EDGE_ATTR, x)


def residual_dropout_ln(x, a, ln: torch.nn.LayerNorm, p: float, training: bool):
    """LN(x + dropout(a, p, training)) with ln's weight / bias / eps."""
    y, edge = _ResidualLayerNormFn.apply(x, a, ln.weight, ln.bias, ln.eps,
                                         float(p), bool(training))
    setattr(y, _EDGE_ATTR, edge)
    return y
