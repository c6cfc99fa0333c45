"""Op dispatch: HIP/CDNA4 kernels on GPU, pure-torch reference on CPU.

On a CUDA(=ROCm) tensor the hand-written gfx950 extension
(oktopk_amd/ops/csrc, built in-tree as oktopk_amd._hip_ops) is REQUIRED —
a missing extension raises instead of silently falling back to eager torch,
so a GPU run can never pass on the slow path unnoticed.  Set
OKTOPK_FORCE_TORCH_OPS=1 to deliberately run the torch reference on GPU
(used by the numerics-oracle tests that compare both).
"""
from __future__ import annotations

import os
from typing import Tuple

import torch

from . import reference as _ref

_FORCE_TORCH = os.environ.get("OKTOPK_FORCE_TORCH_OPS", "0") == "1"
_hip = None
_hip_err: Exception | None = None


def _load_hip():
    global _hip, _hip_err
    if _hip is None and _hip_err is None:
        try:
            from oktopk_amd import _hip_ops  # in-tree built .so

            _hip = _hip_ops
        except ImportError as e:  # remembered; raised on first GPU use
            _hip_err = e
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _backend(t: torch.Tensor):
    if t.is_cuda and not _FORCE_TORCH:
        mod = _load_hip()
        if mod is None:
            raise RuntimeError(
                "oktopk_amd HIP extension (_hip_ops) is not built but a GPU tensor "
                "reached the ops layer. Build it with `python setup.py build_ext "
                "--inplace` (or __graft_entry__.build()). Original import error: "
                f"{_hip_err!r}"
            )
        return mod
    return _ref


# -- public API (signatures documented in ops/reference.py) ----------------

def kth_abs_value(t: torch.Tensor, k: int) -> float:
    return _backend(t).kth_abs_value(t, int(k))


def compact_gt(t: torch.Tensor, tau: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return _backend(t).compact_gt(t, float(tau))


def count_gt(t: torch.Tensor, tau: float) -> int:
    return int(_backend(t).count_gt(t, float(tau)))


def count_multi_gt(t: torch.Tensor, taus) -> list:
    return [int(x) for x in _backend(t).count_multi_gt(t, [float(x) for x in taus])]


def compact_adaptive(t: torch.Tensor, taus, hi_limit: int):
    out = _backend(t).compact_adaptive(t, [float(x) for x in taus], int(hi_limit))
    idx, val, chosen, count = out
    return idx, val, int(chosen), int(count)


def compact_adaptive_ef(t: torch.Tensor, residual: torch.Tensor,
                        grad, taus, hi_limit: int):
    """Fused EF restore (+bf16 upcast when `grad` given) + adaptive-threshold
    compaction: t = float(grad)+residual (or t+=residual), residual = t, and
    select at the first candidate tau whose count fits hi_limit — one
    streaming pass instead of EF + count."""
    aligned = all(
        x is None or x.data_ptr() % 16 == 0 for x in (t, residual, grad)
    ) and (grad is None or grad.dtype == torch.bfloat16)
    if t.is_cuda and not aligned:  # rare: unaligned views fall back unfused
        if grad is not None:
            ef_restore_upcast_(t, residual, grad)
        else:
            ef_restore_snapshot_(t, residual)
        return compact_adaptive(t, taus, hi_limit)
    out = _backend(t).compact_adaptive_ef(
        t, residual, grad, [float(x) for x in taus], int(hi_limit))
    idx, val, chosen, count = out
    return idx, val, int(chosen), int(count)


def gaussian_select_ef(t: torch.Tensor, residual: torch.Tensor, grad,
                       density: float, k: int):
    """Device-resident Gaussian-k selection: residual = float(grad)+residual
    (or t+residual; t itself is NOT written), Gaussian-fit threshold from
    fp64 moments, the three-round refine walk and the extraction at the
    chosen threshold — three tensor-scale passes and one small readback on
    the GPU.  Returns (idx, val, chosen, count, tau, tau0, mean, std) with
    Python scalars; tau == float32(tau0 * GAUSS_FACTORS[chosen])."""
    if grad is not None and grad.dtype != torch.bfloat16:
        raise TypeError("gaussian_select_ef: grad must be bf16 (or None)")
    idx, val, chosen, count, tau, tau0, mean, std = _backend(
        t).gaussian_select_ef(t, residual, grad, float(density), int(k))
    return (idx, val, int(chosen), int(count), float(tau), float(tau0),
            float(mean), float(std))


def _check_select_args(name: str, t: torch.Tensor, k: int, *same) -> None:
    if int(k) < 1:
        raise ValueError(f"{name}: k must be >= 1")
    if t.dtype != torch.float32 or t.dim() != 1 or t.numel() < 1:
        raise TypeError(f"{name}: needs a non-empty 1-D fp32 tensor")
    for x in same:
        if x is not None and (x.device != t.device or x.numel() != t.numel()):
            raise TypeError(f"{name}: device or size mismatch")


def topk_select(t: torch.Tensor, k: int):
    """Exact top-k by magnitude: the min(k, n) largest |t| (abs bit
    pattern), the tie class at the k-th magnitude filled from the lowest
    index.  Returns (idx int32 ascending, val, tau); writes nothing."""
    _check_select_args("topk_select", t, k)
    idx, val, tau = _backend(t).topk_select(t, int(k))
    return idx, val, float(tau)


def topk_select_ef(t: torch.Tensor, residual: torch.Tensor, grad, k: int):
    """topk_select over restored = float(grad)+residual (grad bf16) or
    t+residual, fused with the residual update: residual = restored with
    +0.0 at the selected positions; t is NOT written.  Returns (idx int32
    ascending, val, tau)."""
    _check_select_args("topk_select_ef", t, k, residual, grad)
    if residual.dtype != torch.float32:
        raise TypeError("topk_select_ef: residual must be fp32")
    if grad is not None and grad.dtype != torch.bfloat16:
        raise TypeError("topk_select_ef: grad must be bf16 (or None)")
    idx, val, tau = _backend(t).topk_select_ef(t, residual, grad, int(k))
    return idx, val, float(tau)


def sparse_merge_topk(a_idx: torch.Tensor, a_val: torch.Tensor,
                      b_idx: torch.Tensor, b_val: torch.Tensor, k: int):
    """Top-k of a + b for two sparse vectors (int32 indices ascending and
    unique, fp32 values; either may be empty): union over indices, values
    summed where both hold one, the min(k, |union|) largest |v| kept with
    topk_select's tie rule.  Returns (idx ascending, val).  Work is
    O((|a|+|b|) log), independent of the dense length."""
    if int(k) < 1:
        raise ValueError("sparse_merge_topk: k must be >= 1")
    for i, v in ((a_idx, a_val), (b_idx, b_val)):
        if (i.dtype != torch.int32 or v.dtype != torch.float32
                or i.dim() != 1 or i.shape != v.shape):
            raise TypeError("sparse_merge_topk: needs 1-D (int32 idx, fp32 "
                            "val) pairs of equal length")
        if i.device != a_idx.device or v.device != a_idx.device:
            raise TypeError("sparse_merge_topk: device mismatch")
    return tuple(_backend(a_val).sparse_merge_topk(a_idx, a_val, b_idx, b_val,
                                                   int(k)))


def scatter_add_(dest: torch.Tensor, idx: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    return _backend(dest).scatter_add_(dest, idx, val)


def zero_at_(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return _backend(t).zero_at_(t, idx)


def zero_at_masked_(t: torch.Tensor, idx: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    return _backend(t).zero_at_masked_(t, idx, mask)


def fill_sparse_scaled_(
    out: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, scale: float
) -> torch.Tensor:
    return _backend(out).fill_sparse_scaled_(out, idx, val, float(scale))


def isin_sorted(a: torch.Tensor, b_sorted: torch.Tensor) -> torch.Tensor:
    return _backend(a).isin_sorted(a, b_sorted)


def ef_restore_snapshot_(t: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    return _backend(t).ef_restore_snapshot_(t, residual)


def ef_restore_upcast_(t: torch.Tensor, residual: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    return _backend(t).ef_restore_upcast_(t, residual, g)


def fused_sgd_(param, grad, momentum_buf, lr, momentum, weight_decay, nesterov):
    return _backend(param).fused_sgd_(
        param, grad, momentum_buf, float(lr), float(momentum), float(weight_decay), bool(nesterov)
    )


def fused_adam_(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                weight_decay, gscale=None):
    return _backend(param).fused_adam_(
        param, grad, exp_avg, exp_avg_sq, float(lr), float(beta1), float(beta2),
        float(eps), float(weight_decay), gscale
    )


def fused_adam_mirror_(param, grad, exp_avg, exp_avg_sq, param_bf16, lr, beta1,
                       beta2, eps, weight_decay, gscale=None):
    """Adam step + bf16 weight-mirror write in one pass (GPU); CPU reference
    steps then casts.  `gscale` (optional 1-elem tensor) pre-scales the
    gradient read — the device-resident grad clip."""
    b = _backend(param)
    if hasattr(b, "fused_adam_mirror_"):
        return b.fused_adam_mirror_(
            param, grad, exp_avg, exp_avg_sq, param_bf16, float(lr), float(beta1),
            float(beta2), float(eps), float(weight_decay), gscale
        )
    b.fused_adam_(param, grad, exp_avg, exp_avg_sq, float(lr), float(beta1),
                  float(beta2), float(eps), float(weight_decay), gscale)
    param_bf16.copy_(param)


def scatter_gt_credit_(result, residual, idx, val, tau, scale=1.0) -> int:
    """Fused world-1 round-2 tail: where |val|>tau, result[idx]=val*scale
    and residual[idx]=0; returns the selected count.  `result` must be
    zeroed by the caller; `result=None` does the credit and the count only
    (the sparse optimizer tail below needs no dense gradient)."""
    if result is None:
        return int(_backend(residual).credit_gt_(residual, idx, val, float(tau)))
    return int(_backend(result).scatter_gt_credit_(
        result, residual, idx, val, float(tau), float(scale)))


# -- sparse optimizer tail ---------------------------------------------------
# A sparse gradient (idx int32 ascending+unique, val fp32, scale, tau) stands
# for the dense vector that is val[i]*scale at idx[i] where |val[i]| > tau
# (tau < 0 keeps every entry) and +0.0 elsewhere: what fill_sparse_scaled_,
# or zero + scatter_gt_credit_, would have written.

def sparse_sumsq_into_(acc: torch.Tensor, idx, val, scale: float,
                       tau: float, n=None) -> None:
    """acc (fp64[1], same device) += sum of squares of the dense gradient a
    sparse one stands for; no host sync on GPU.  With `n` (the dense length)
    the CPU reference densifies and sums in the dense route's order, as
    grad_clip_scale_sparse does; the HIP op ignores it."""
    b = _backend(val)
    if b is _ref and n is not None:
        return b.sumsq_into_(acc, b.densify_sparse_grad(
            idx, val, 0, int(n), float(scale), float(tau)))
    return b.sparse_sumsq_into_(acc, idx, val, float(scale), float(tau))


def grad_clip_scale_sparse(idx, val, scale: float, tau: float,
                           max_norm: float, n: int) -> torch.Tensor:
    """grad_clip_scale of the length-n dense gradient, from its sparse form;
    no host sync.  The HIP op sums the kept entries in fp64 (n unused); the
    CPU reference densifies to sum in the dense route's order."""
    b = _backend(val)
    if b is _ref:
        return b.grad_clip_scale_sparse(idx, val, float(scale), float(tau),
                                        float(max_norm), int(n))
    return b.grad_clip_scale_sparse(idx, val, float(scale), float(tau),
                                    float(max_norm))


def fused_adam_sparse_(param, idx, val, base, scale, tau, exp_avg, exp_avg_sq,
                       lr, beta1, beta2, eps, weight_decay, gscale=None):
    """fused_adam_ on the slice [base, base+len(param)) of a sparse gradient:
    bit-identical to densifying first, without the dense read."""
    return _backend(param).fused_adam_sparse_(
        param, idx, val, int(base), float(scale), float(tau), exp_avg,
        exp_avg_sq, float(lr), float(beta1), float(beta2), float(eps),
        float(weight_decay), gscale)


def fused_adam_sparse_mirror_(param, idx, val, base, scale, tau, exp_avg,
                              exp_avg_sq, param_bf16, lr, beta1, beta2, eps,
                              weight_decay, gscale=None):
    """fused_adam_sparse_ + bf16 weight-mirror write in one pass (GPU); the
    CPU reference steps then casts."""
    b = _backend(param)
    if hasattr(b, "fused_adam_sparse_mirror_"):
        return b.fused_adam_sparse_mirror_(
            param, idx, val, int(base), float(scale), float(tau), exp_avg,
            exp_avg_sq, param_bf16, float(lr), float(beta1), float(beta2),
            float(eps), float(weight_decay), gscale)
    b.fused_adam_sparse_(param, idx, val, int(base), float(scale), float(tau),
                         exp_avg, exp_avg_sq, float(lr), float(beta1),
                         float(beta2), float(eps), float(weight_decay), gscale)
    param_bf16.copy_(param)


# -- flat SGD ------------------------------------------------------------------

def sgd_step_(param, grad, momentum_buf, lr, momentum, weight_decay, nesterov,
              gscale=None):
    """SGD step (momentum / nesterov / weight decay, no dampening) over flat
    fp32 tensors, every multiply and add rounded separately (the contract is
    in ops/reference.py).  `gscale` (optional 1-elem tensor) pre-scales the
    gradient read — the device-resident grad clip.  `momentum_buf` is not
    touched when momentum == 0 and may then be empty."""
    return _backend(param).sgd_step_(
        param, grad, momentum_buf, float(lr), float(momentum),
        float(weight_decay), bool(nesterov), gscale)


def sgd_step_sparse_(param, idx, val, base, scale, tau, momentum_buf, lr,
                     momentum, weight_decay, nesterov, gscale=None):
    """sgd_step_ on the slice [base, base+len(param)) of a sparse gradient:
    bit-identical to fill_sparse_scaled_ + sgd_step_, without the zero fill,
    the scatter and the dense gradient read.  Entries outside the slice are
    ignored."""
    return _backend(param).sgd_step_sparse_(
        param, idx, val, int(base), float(scale), float(tau), momentum_buf,
        float(lr), float(momentum), float(weight_decay), bool(nesterov),
        gscale)


def clip_scale_from_sumsq(acc: torch.Tensor, max_norm: float) -> torch.Tensor:
    """grad_clip_scale's factor from an fp64[1] sum of squares accumulated
    with sumsq_into_ / sparse_sumsq_into_ (one accumulator may span several
    buffers); a 1-elem fp32 tensor on acc's device, no host sync."""
    return _backend(acc).clip_scale_from_sumsq(acc, float(max_norm))


# -- sparse wire codec ([idx int32 | val bits] per segment, fp32 or bf16) ---
# The HIP kernels keep their segment tables in LDS and take a bounded number
# of segments; beyond it the torch reference runs on the same device (a
# world that large is far outside anything the kernels were sized for).

def _wire_backend(t: torch.Tensor, nseg: int):
    b = _backend(t)
    if b is not _ref and nseg > b.wire_max_segments():
        return _ref
    return b


def pack_regions(idx: torch.Tensor, val: torch.Tensor, bounds: torch.Tensor,
                 wire_bf16: bool):
    """Split the ascending selection at the [P+1] int64 CPU `bounds`
    (segment j: bounds[j] <= idx < bounds[j+1]) and pack it into the wire
    layout.  Returns (buf int32 on idx.device, counts: list of P ints)."""
    buf, counts = _wire_backend(idx, bounds.numel() - 1).pack_regions(
        idx, val, bounds, bool(wire_bf16))
    return buf, [int(c) for c in counts]


def unpack_segments(buf: torch.Tensor, counts, wire_bf16: bool):
    """All wire segments gathered into contiguous (idx int32, val fp32)."""
    counts = [int(c) for c in counts]
    idx, val = _wire_backend(buf, len(counts)).unpack_segments(
        buf, counts, bool(wire_bf16))
    return idx, val


def unpack_scatter_add_(dest: torch.Tensor, buf: torch.Tensor, counts,
                        base: int, wire_bf16: bool) -> torch.Tensor:
    """dest[idx - base] += val for every wire entry, without materialising
    the unpacked segments (GPU).  base <= idx < base + dest.numel()."""
    counts = [int(c) for c in counts]
    return _wire_backend(dest, len(counts)).unpack_scatter_add_(
        dest, buf, counts, int(base), bool(wire_bf16))


# -- Ok-Topk round-2 tail: global selection + residual credit ----------------

def _check_round2_args(name: str, residual, idx, k, *i32f32) -> None:
    if k is not None and int(k) < 1:
        raise ValueError(f"{name}: k must be >= 1")
    if residual.dtype != torch.float32 or residual.dim() != 1:
        raise ValueError(f"{name}: residual must be a 1-D fp32 tensor")
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise ValueError(f"{name}: idx must be a 1-D int32 tensor")
    for x, dt in i32f32:
        if x.dtype != dt or x.dim() != 1:
            raise ValueError(f"{name}: needs 1-D int32 index / wire words "
                             "and fp32 values")
    for x in (idx,) + tuple(x for x, _ in i32f32):
        if x.device != residual.device:
            raise ValueError(f"{name}: device mismatch")


def round2_tail_(residual: torch.Tensor, idx: torch.Tensor,
                 all_idx: torch.Tensor, all_val: torch.Tensor, k=None):
    """Round-2 tail of Ok-Topk over the gathered survivors (all_idx int32
    ascending and unique, all_val fp32) and the local selection idx (int32
    ascending, unique).  k None, or nothing gathered: the selection is every
    gathered entry, returned as passed in, tau None.  k given: the
    min(k, S) largest |all_val| under topk_select's rule, g_idx ascending,
    tau the k-th magnitude.  Either way residual[j] = +0.0 for every j in
    both g_idx and idx and nothing else is written.  Returns (g_idx, g_val,
    tau)."""
    _check_round2_args("round2_tail_", residual, idx, k,
                       (all_idx, torch.int32), (all_val, torch.float32))
    if all_idx.numel() != all_val.numel():
        raise ValueError("round2_tail_: all_idx / all_val length mismatch")
    g_idx, g_val, tau = _backend(residual).round2_tail_(
        residual, idx, all_idx, all_val, None if k is None else int(k))
    return g_idx, g_val, None if tau is None else float(tau)


def round2_tail_wire_(residual: torch.Tensor, idx: torch.Tensor,
                      buf: torch.Tensor, counts, wire_bf16: bool, k=None):
    """round2_tail_ with the gathered survivors given as the allgathered
    wire buffer (`counts`: element counts per rank segment): bit-equal to
    round2_tail_ over unpack_segments(buf, counts, wire_bf16), decoded in
    the same kernels on the GPU.  With k=None the returned pair is the
    unpacked lists."""
    counts = [int(c) for c in counts]
    _check_round2_args("round2_tail_wire_", residual, idx, k,
                       (buf, torch.int32))
    if any(c < 0 for c in counts) or sum(
            _ref._wire_words(c, bool(wire_bf16)) for c in counts) > buf.numel():
        raise ValueError("round2_tail_wire_: counts do not fit the buffer")
    g_idx, g_val, tau = _wire_backend(residual, len(counts)).round2_tail_wire_(
        residual, idx, buf, counts, bool(wire_bf16),
        None if k is None else int(k))
    return g_idx, g_val, None if tau is None else float(tau)


# -- Ok-Topk round-1 reduce: ordered sparse merge at the region owner ---------
# The HIP kernels rank every entry by one binary search per other segment, so
# the device path takes a bounded number of segments; beyond it the torch
# reference runs on the same device, as for the wire codec.

def reduce_max_segments() -> int:
    """Largest segment count the HIP reduce takes (RM_MAX_SEG of
    reduce_merge.hip; the reference has no limit).  Needs the extension."""
    mod = _load_hip()
    if mod is None:
        raise RuntimeError(f"oktopk_amd HIP extension is not built: {_hip_err!r}")
    return int(mod.reduce_max_segments())


def _reduce_backend(t: torch.Tensor, nseg: int):
    b = _backend(t)
    if b is not _ref and nseg > b.reduce_max_segments():
        return _ref
    return b


def _check_reduce_args(name: str, counts, base, length, tau, *i32f32) -> None:
    for x, dt in i32f32:
        if x.dtype != dt or x.dim() != 1:
            raise ValueError(f"{name}: needs 1-D int32 index / wire words "
                             "and fp32 values")
        if x.device != i32f32[0][0].device:
            raise ValueError(f"{name}: device mismatch")
    if any(c < 0 for c in counts):
        raise ValueError(f"{name}: negative segment count")
    if not float(tau) >= 0.0:
        raise ValueError(f"{name}: tau must be >= 0")
    if int(length) < 0:
        raise ValueError(f"{name}: length must be >= 0")


def reduce_segments(idx: torch.Tensor, val: torch.Tensor, counts, base: int,
                    length: int, tau: float):
    """Round-1 reduce of Ok-Topk at a region owner.  idx (int32) / val
    (fp32) hold len(counts) concatenated segments in rank order, each
    ascending and duplicate-free.  Entries with base <= idx < base + length
    are summed per index in segment order, one fp32 add each — ((v_a + v_b)
    + v_c) ..., the order of index_add_ on the CPU — and the indices with
    |sum| > tau (tau >= 0) come back ascending as (g_idx int32, g_val).
    Bit-equal to zeros(length) + scatter_add_ + compact_gt + base on the
    CPU for NaN-free sums (a NaN sum is dropped here, float comparison, and
    kept by compact_gt's bit rule); on the GPU nothing of size `length` is
    touched and no float atomic runs, so the result is the same on every
    run."""
    counts = [int(c) for c in counts]
    _check_reduce_args("reduce_segments", counts, base, length, tau,
                       (idx, torch.int32), (val, torch.float32))
    if idx.numel() != val.numel():
        raise ValueError("reduce_segments: idx / val length mismatch")
    if sum(counts) != idx.numel():
        raise ValueError("reduce_segments: counts do not sum to idx.numel()")
    return tuple(_reduce_backend(idx, len(counts)).reduce_segments(
        idx, val, counts, int(base), int(length), float(tau)))


def reduce_segments_wire(buf: torch.Tensor, counts, wire_bf16: bool, base: int,
                         length: int, tau: float):
    """reduce_segments with the segments still packed in the wire layout
    (`counts`: element counts per segment): bit-equal to reduce_segments
    over unpack_segments(buf, counts, wire_bf16), decoded in the same
    kernels on the GPU with no unpacked copy."""
    counts = [int(c) for c in counts]
    _check_reduce_args("reduce_segments_wire", counts, base, length, tau,
                       (buf, torch.int32))
    if sum(_ref._wire_words(c, bool(wire_bf16)) for c in counts) > buf.numel():
        raise ValueError("reduce_segments_wire: counts do not fit the buffer")
    return tuple(_reduce_backend(buf, len(counts)).reduce_segments_wire(
        buf, counts, bool(wire_bf16), int(base), int(length), float(tau)))


def grad_clip_scale(t: torch.Tensor, max_norm: float) -> torch.Tensor:
    """Device-resident clip factor: min(1, max/(||t||+1e-6)) as a 1-elem
    tensor, no host sync (feeds fused_adam_'s gscale)."""
    return _backend(t).grad_clip_scale(t, float(max_norm))


def sumsq_into_(acc: torch.Tensor, t: torch.Tensor) -> None:
    """acc (fp64[1], same device) += sum(t^2); no host sync on GPU."""
    return _backend(t).sumsq_into_(acc, t)


def l2norm(t: torch.Tensor) -> float:
    return float(_backend(t).l2norm(t))
