"""LayerNorm whose backward writes the gamma/beta gradients into bound
gradient slots (the LayerNorm counterpart of the direct-gradient Linear in
fused_linear.py; same binding protocol, same first-write-overwrites rule).

Forward is torch's native_layer_norm, unchanged, keeping its mean / rstd.
Backward is two kernels of ours (ops/csrc/ln_bwd.hip): gx plus per-block
fp32 partial sums, then a fixed-order reduction that stores bf16 into the
two slots.  That replaces torch's LayerNorm-backward kernels plus the two
autograd accumulate adds per site.  Hidden sizes the kernel does not handle,
unbound parameters, CPU / fp32: torch's native_layer_norm_backward with
ordinary returned gradients.

Opt-in with OKTOPK_DIRECT_LN=1 (see profiles/README.md r03 for the A/B that
decides the default); only consulted when the model is built.
"""
from __future__ import annotations

import os

import torch

from .fused_linear import _SLOT_ATTR, _bound_slot


def direct_ln_enabled() -> bool:
    return os.environ.get("OKTOPK_DIRECT_LN", "0") == "1"


class _SlotLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        y, mean, rstd = torch.native_layer_norm(x, (x.shape[-1],), w, b, eps)
        ctx.save_for_backward(x, w, b, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, b, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        H = x.shape[-1]
        ws, bs = _bound_slot(w), _bound_slot(b)
        if (ws is not None and bs is not None and ws[1] is bs[1]
                and need[1] and need[2]
                and gy.is_cuda and gy.dtype == torch.bfloat16
                and x.dtype == torch.bfloat16):
            from oktopk_amd import _hip_ops

            owner = ws[1]
            w_acc, b_acc = id(w) in owner.written, id(b) in owner.written
            if w_acc == b_acc and _hip_ops.ln_bwd_supported(H):
                gx = _hip_ops.ln_bwd_into(gy, x, w, mean, rstd, ws[0], bs[0], w_acc)
                owner.written.update((id(w), id(b)))
                return gx, None, None, None
        gx, gw, gb = torch.ops.aten.native_layer_norm_backward(
            gy.contiguous(), x, [H], mean, rstd, w, b,
            [bool(need[0]), bool(need[1]), bool(need[2])])
        return gx, gw, gb, None


class SlotLayerNorm(torch.nn.LayerNorm):
    """Drop-in nn.LayerNorm (same state_dict keys); runs the node above only
    while its parameters are bound to gradient slots."""

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.bfloat16 and torch.is_grad_enabled()
                and self.elementwise_affine and self.bias is not None
                and len(self.normalized_shape) == 1
                and hasattr(self.weight, _SLOT_ATTR)):
            return _SlotLayerNormFn.apply(x, self.weight, self.bias, self.eps)
        return super().forward(x)
