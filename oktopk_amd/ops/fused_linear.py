"""Fused Linear+GELU (hand-written MFMA kernel) with autograd.

The forward runs the CDNA4 kernel (ops/csrc/linear_gelu.hip): one launch for
GEMM + bias + erf-GELU, also materialising the pre-activation for backward.
Backward uses the saved pre-activation for the exact erf-GELU derivative and
rocBLAS matmuls for the two gradient GEMMs.

Further down: the direct-gradient Linear node (backward writes gW / gb into
the optimizer's flat gradient buffer, native linear_bwd_into) and
ColsumLinear, the nn.Linear every BERT site uses.

Parity: the reference's LinearActivation fused-gelu module
(/root/reference/BERT/bert/transformers/modeling.py:75).
"""
from __future__ import annotations

import os

import torch

_SQRT1_2 = 0.7071067811865476
_INV_SQRT_2PI = 0.3989422804014327


def fused_available(x: torch.Tensor, weight: torch.Tensor) -> bool:
    # opt-in: at BERT-base shapes (M=1024, 192 blocks) the correctness-tier
    # kernel underfills 256 CUs and loses ~1ms/step to hipBLASLt+gelu
    # (measured); enable for A/B with OKTOPK_FUSED_MLP=1
    if os.environ.get("OKTOPK_FUSED_MLP", "0") != "1":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16):
        return False
    if weight.shape[1] % 32 != 0:
        return False
    from . import hip_available

    return hip_available()


class _FusedLinearGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        from oktopk_amd import _hip_ops

        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        b = bias if bias is not None else torch.empty(0, device=x.device)
        y, z = _hip_ops.linear_gelu(x2, weight.contiguous(), b, True, True)
        ctx.save_for_backward(x2, weight, z, bias)
        ctx.in_shape = shp
        return y.reshape(*shp[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, w, z, b = ctx.saved_tensors
        gy2 = gy.reshape(-1, gy.shape[-1])
        zf = z.float()
        # d/dz gelu_erf(z) = Phi(z) + z * phi(z)
        gp = 0.5 * (1.0 + torch.erf(zf * _SQRT1_2)) + zf * torch.exp(-0.5 * zf * zf) * _INV_SQRT_2PI
        gpre = (gy2.float() * gp).to(gy2.dtype)
        gx, gw, gb = linear_param_grads(gpre, x2, w, b, ctx.needs_input_grad[1],
                                        b is not None and ctx.needs_input_grad[2])
        return gx.reshape(ctx.in_shape), gw, gb


def fused_linear_gelu(x: torch.Tensor, weight: torch.Tensor, bias=None) -> torch.Tensor:
    """y = gelu(x @ weight^T + bias), bf16, single MFMA kernel forward."""
    return _FusedLinearGelu.apply(x, weight, bias)


# ---------------------------------------------------------------------------
# Direct-gradient Linear: backward writes gW and gb straight into the
# optimizer's flat gradient buffer.
#
# FlatBertAdam aliases every p.grad to a slice ("slot") of one flat buffer.
# With plain autograd each Linear then costs, per parameter and per step, a
# temporary gradient plus an accumulate kernel `slot += g` onto a slot that
# zero_grad() just zeroed.  Here the weight-gradient GEMM has the slot as its
# output and the bias gradient is a column reduction whose output is the slot
# (the one-launch kernel that sums in torch's order, bit-identical to torch's
# own reduction; see bias_grad_mode for the switch), and the node hands
# autograd an undefined gradient for both, so its accumulate step has nothing
# to do.
#
# Protocol (three attributes on the Parameter, nothing else is shared):
#   * the MODEL calls mark_every_backward(p) on parameters whose Linear runs
#     in every backward pass — only those may skip zeroing;
#   * the OPTIMIZER that owns the flat buffer calls bind_grad_slot(p, slot,
#     owner) for the marked parameters it aliases;
#   * the NODE, at backward time, re-checks that p.grad still IS that slot
#     (same storage address, contiguous, same dtype).  Anything else — no
#     binding, a hook-driven optimizer that re-pointed .grad, .grad = None —
#     gets ordinary returned gradients, exactly what F.linear's autograd
#     gives.
# The first write of a slot after zero_grad() overwrites it; a further write
# before the next zero_grad() (gradient accumulation, a weight used twice)
# accumulates (GEMM beta = 1).  owner.written records which is which.
# ---------------------------------------------------------------------------

_SLOT_ATTR = "_oktopk_grad_slot"
_EVERY_BWD_ATTR = "_oktopk_every_backward"


def bias_grad_mode() -> str:
    """Which column reduction writes a bound bias-gradient slot.

    OKTOPK_COLSUM_BIAS unset -> "exact": the one-launch kernel that adds in
        the order of torch's reduce_kernel and so leaves torch's bits; shapes
        or devices outside the ported configuration run torch's reduction.
    =0 -> "torch": torch's reduction everywhere (semaphore memset, 32 blocks
        per strip and a global combine for 1.5 MB: ~16 us per bias).
    =1 -> "fast": the older one-launch kernel with its own order.  Once in
        some million elements it rounds to the neighbouring bf16, which is
        enough to move a training run onto another trajectory."""
    v = os.environ.get("OKTOPK_COLSUM_BIAS")
    if v == "1":
        return "fast"
    if v == "0":
        return "torch"
    return "exact"


def direct_grad_enabled() -> bool:
    """OKTOPK_DIRECT_GRAD=0 restores zero + autograd-accumulate everywhere."""
    return os.environ.get("OKTOPK_DIRECT_GRAD", "1") != "0"


class GradSlotOwner:
    """Per-optimizer state the nodes share: ids of the parameters whose slot
    was written since the last zero_grad()."""

    def __init__(self):
        self.written = set()


def mark_every_backward(p: torch.Tensor) -> None:
    """Model-side promise: the Linear using `p` runs in every backward of
    the model, so its slot is always rewritten and needs no zeroing."""
    setattr(p, _EVERY_BWD_ATTR, True)


def runs_every_backward(p: torch.Tensor) -> bool:
    return bool(getattr(p, _EVERY_BWD_ATTR, False))


def bind_grad_slot(p: torch.Tensor, slot: torch.Tensor, owner: GradSlotOwner) -> None:
    setattr(p, _SLOT_ATTR, (slot, owner))


def unbind_grad_slot(p: torch.Tensor) -> None:
    if hasattr(p, _SLOT_ATTR):
        delattr(p, _SLOT_ATTR)


def _bound_slot(p):
    """(grad, owner) if p.grad is still the bound slot, else None."""
    bound = getattr(p, _SLOT_ATTR, None)
    if bound is None:
        return None
    slot, owner = bound
    g = p.grad
    if (g is None or g.data_ptr() != slot.data_ptr() or g.shape != p.shape
            or g.dtype != p.dtype or g.dtype != torch.bfloat16
            or not g.is_cuda or not g.is_contiguous()):
        return None
    return g, owner


def linear_param_grads(gy, x, w, b, need_w=True, need_b=True, w_shared=False):
    """Backward of y = x W^T + b.  Returns (gx, gw, gb); gw / gb are None
    when they were written into the parameter's bound gradient slot.

    w_shared: the weight has another user in the same backward (a tied
    weight), whose gradient autograd adds onto the slot after this node's
    write.  That is exact for the overwriting first write.  Once the slot
    holds an earlier sub-step's sum, adding the two users' gradients one at
    a time rounds differently from the plain path wherever they nearly
    cancel, so from then on gW is returned and autograd adds the SUM of both
    in one rounding, as it always did."""
    gy2 = gy.reshape(-1, gy.shape[-1])
    x2 = x.reshape(-1, x.shape[-1])
    ws = bs = None
    if gy.is_cuda and gy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16:
        ws = _bound_slot(w) if need_w else None
        bs = _bound_slot(b) if (need_b and b is not None) else None
        if w_shared and ws is not None and id(w) in ws[1].written:
            ws = None
    if ws is None and bs is None:
        gx = (gy2 @ w).reshape(x.shape)
        gw = gy2.t() @ x2 if need_w else None
        gb = gy2.sum(0) if (need_b and b is not None) else None
        return gx, gw, gb

    from oktopk_amd import _hip_ops

    owner = (ws or bs)[1]
    # Every gradient stays bit-identical to the zero + accumulate path: the
    # default bias reduction is the one-launch kernel in torch's summation
    # order (bias_grad_mode above; "fast" is the opt-in that is not).
    mode = bias_grad_mode()
    bias_kernel, bias_exact = mode == "fast", mode == "exact"
    keys = [id(p) for p, s in ((w, ws), (b, bs)) if s is not None]
    accumulate = all(k in owner.written for k in keys)
    if not accumulate and any(k in owner.written for k in keys):
        # mixed state (a bias shared without its weight): one call each
        gx = _hip_ops.linear_bwd_into(gy, x, w, ws[0] if ws else None, None,
                                      id(w) in owner.written, False)
        if bs is not None:
            _hip_ops.linear_bwd_into(gy, x, w, None, bs[0],
                                     id(b) in owner.written, bias_kernel,
                                     bias_exact)
    else:
        gx = _hip_ops.linear_bwd_into(gy, x, w, ws[0] if ws else None,
                                      bs[0] if bs else None, accumulate,
                                      bias_kernel, bias_exact)
    owner.written.update(keys)
    gw = gy2.t() @ x2 if (need_w and ws is None) else None
    gb = gy2.sum(0) if (need_b and b is not None and bs is None) else None
    return gx, gw, gb


class _DirectGradLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, w_shared=False):
        # w and b are leaves: saved_tensors hands back the Parameters
        # themselves, so backward can look at their .grad
        ctx.save_for_backward(x, w, b)
        ctx.w_shared = w_shared
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        x, w, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gw, gb = linear_param_grads(gy, x, w, b, need[1],
                                        b is not None and need[2],
                                        ctx.w_shared)
        return (gx if need[0] else None), gw, gb, None


def direct_linear(x, w, b=None, w_shared=False):
    """F.linear whose backward writes gW / gb into bound gradient slots.
    The weight stays a differentiable input of the node: for a tied weight
    (BERT's decoder shares the word-embedding matrix; pass w_shared=True)
    autograd then orders the other user's accumulate `slot += g` after this
    node's overwrite."""
    if (x.is_cuda and x.dtype == torch.bfloat16 and torch.is_grad_enabled()
            and (hasattr(w, _SLOT_ATTR) or (b is not None and hasattr(b, _SLOT_ATTR)))):
        return _DirectGradLinear.apply(x, w, b, w_shared)
    return torch.nn.functional.linear(x, w, b)


# ---------------------------------------------------------------------------
# ColsumLinear: nn.Linear routed through the direct-gradient node when its
# parameters are bound to gradient slots.  Unbound, OKTOPK_COLSUM_BIAS=1
# still swaps torch's bias-gradient reduce_kernel (~10 us each in the r02-i
# profile) for the one-launch column-sum kernel, with ordinary returned
# gradients; the input/weight gradients are the same two GEMMs torch runs.
# ---------------------------------------------------------------------------

class _LinearColsumBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, gy):
        from oktopk_amd import _hip_ops

        x, w = ctx.saved_tensors
        gy_c = gy.contiguous()
        gx = gy_c @ w
        gy2 = gy_c.reshape(-1, gy_c.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        gw = gy2.t() @ x2
        gb = torch.empty(gy2.shape[-1], dtype=gy2.dtype, device=gy2.device)
        _hip_ops.colsum_bf16_into(gy2, gb, False)
        return gx, gw, gb


class ColsumLinear(torch.nn.Linear):
    """Drop-in nn.Linear (same state_dict keys).

    Bound to gradient slots (FlatBertAdam, OKTOPK_DIRECT_GRAD != 0) it runs
    the direct-gradient node above.  Otherwise it is F.linear, or with
    OKTOPK_COLSUM_BIAS=1 the kernel bias-gradient path.  History of that
    switch: its first version (r02-r) measured 9.27-9.31 vs 9.24-9.25
    ms/step, neutral to negative — but it replaced torch's single reduce
    kernel with three launches (zeros, fp32-atomics kernel, cast) and its
    result still went through autograd's accumulate add, so it never tested
    whether removing kernels pays.  The switch now selects the one-launch
    kernel, in the bound node too; it is opt-in because its summation
    order differs from torch's in rare last-bit roundings
    (profiles/README.md r03).  The bound node's default is since r07 the
    one-launch kernel that follows torch's order (bias_grad_mode), which
    takes the launches away without moving a bit."""

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.bfloat16
                and self.weight.dtype == torch.bfloat16):
            if hasattr(self.weight, _SLOT_ATTR) and torch.is_grad_enabled():
                return _DirectGradLinear.apply(x, self.weight, self.bias, False)
            if (self.bias is not None
                    and os.environ.get("OKTOPK_COLSUM_BIAS", "0") == "1"):
                from . import hip_available

                if hip_available():
                    return _LinearColsumBias.apply(x, self.weight, self.bias)
        return torch.nn.functional.linear(x, self.weight, self.bias)
