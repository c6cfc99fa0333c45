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

Without that opt-in, an optimizer that defers small gradient writes
(GradSlotOwner in fused_linear.py, OKTOPK_DEFER_SMALL_GRADS) binds gamma and
beta as add slots.  The node then runs torch's own
native_layer_norm_backward for all three gradients, so every bit is torch's,
hands autograd no gamma / beta gradient, and leaves the two `slot += g` adds
to the batched launch at the end of the backward pass.  With 128 to 1024
rows (and not OKTOPK_BATCH_LN_GRADS=0) the node calls torch for the input
gradient only: the gamma / beta reductions wait for the end of the pass
too, where one launch (ops/csrc/ln_param_grads.hip) computes them for every
site in torch's summation order and adds them onto the slots.
"""
from __future__ import annotations

import os

import torch

from .fused_linear import (_ADD_SLOT_ATTR, _SLOT_ATTR, LnGradSource, _bound_slot,
                           batch_ln_grads_enabled, defer_small_grads_enabled)


def direct_ln_enabled() -> bool:
    return os.environ.get("OKTOPK_DIRECT_LN", "0") == "1"


def _add_slots(w, b):
    """(gamma slot, beta slot, owner) when both are bound as add slots of one
    owner and deferral is on, else None."""
    if not defer_small_grads_enabled():
        return None
    was, bas = _bound_slot(w, _ADD_SLOT_ATTR), _bound_slot(b, _ADD_SLOT_ATTR)
    if was is None or bas is None or was[1] is not bas[1]:
        return None
    return was[0], bas[0], was[1]


def defer_ln_param_grads(w, b, gw, gb) -> bool:
    """Hand torch's gamma / beta gradients to the parameters' add slots, to be
    added by the batched launch at the end of backward.  False: not bound as
    add slots of one owner (or deferral is off); return them to autograd."""
    slots = _add_slots(w, b)
    if (slots is not None
            and gw.dtype == torch.bfloat16 and gb.dtype == torch.bfloat16
            and gw.is_contiguous() and gb.is_contiguous()):
        slots[2].defer(w, gw, slots[0], False)
        slots[2].defer(b, gb, slots[1], False)
        return True
    return False


def defer_ln_param_grad_sums(w, b, gy, x, mean, rstd) -> bool:
    """Leave the gamma / beta gradients of this site to the batched launch at
    the end of backward, which computes them with torch's bits and adds them
    onto the slots (OKTOPK_BATCH_LN_GRADS).  False: the switch is off, the
    parameters are not add slots of one owner, the shape is outside what the
    kernel reproduces, or a parameter already has a pending entry (a module
    used twice); the caller then computes them with torch, as before."""
    if not batch_ln_grads_enabled():
        return False
    slots = _add_slots(w, b)
    if slots is None or slots[2].has_pending(w) or slots[2].has_pending(b):
        return False
    from oktopk_amd import _hip_ops

    if not _hip_ops.ln_param_grads_deferrable(gy, x, mean, rstd):
        return False
    slots[2].defer_ln(LnGradSource(gy, x, mean, rstd, w, b, slots[0], slots[1]))
    return True


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
        gy = gy.contiguous()
        if need[1] and need[2] and defer_ln_param_grad_sums(w, b, gy, x, mean, rstd):
            gx = None
            if need[0]:
                gx = torch.ops.aten.native_layer_norm_backward(
                    gy, x, [H], mean, rstd, w, b, [True, False, False])[0]
            return gx, None, None, None
        gx, gw, gb = torch.ops.aten.native_layer_norm_backward(
            gy, x, [H], mean, rstd, w, b,
            [bool(need[0]), bool(need[1]), bool(need[2])])
        if need[1] and need[2] and defer_ln_param_grads(w, b, gw, gb):
            return gx, None, None, None
        return gx, gw, gb, None


class SlotLayerNorm(torch.nn.LayerNorm):
    """Drop-in nn.LayerNorm (same state_dict keys); runs the node above only
    while its parameters are bound to gradient slots."""

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.bfloat16 and torch.is_grad_enabled()
                and self.elementwise_affine and self.bias is not None
                and len(self.normalized_shape) == 1
                and (hasattr(self.weight, _SLOT_ATTR)
                     or hasattr(self.weight, _ADD_SLOT_ATTR))):
            return _SlotLayerNormFn.apply(x, self.weight, self.bias, self.eps)
        return super().forward(x)
