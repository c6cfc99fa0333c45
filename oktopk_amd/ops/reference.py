"""Pure-PyTorch reference implementations of every engine op.

These are the numerics oracle for the HIP/CDNA4 kernels (tests compare the
kernels against these in fp32) and the CPU execution path (gloo CI).  Each op
mirrors a torch/numpy call-site of the reference implementation — citations on
each function point into /root/reference.

Contract shared with the HIP backend (oktopk_amd/ops/csrc):
  * gradients / dense tensors: 1-D contiguous fp32 (or bf16 where noted)
  * index vectors: int32, ascending order when produced by compact_gt
"""
from __future__ import annotations

import collections
import math
from typing import Tuple

import torch

__all__ = [
    "kth_abs_value",
    "compact_gt",
    "count_gt",
    "count_multi_gt",
    "compact_adaptive",
    "gaussian_select_ef",
    "topk_select",
    "topk_select_ef",
    "sparse_merge_topk",
    "scatter_add_",
    "zero_at_",
    "zero_at_masked_",
    "fill_sparse_scaled_",
    "isin_sorted",
    "ef_restore_snapshot_",
    "ef_restore_upcast_",
    "fused_sgd_",
    "fused_adam_",
    "l2norm",
    "pack_regions",
    "unpack_segments",
    "unpack_scatter_add_",
    "reduce_segments",
    "reduce_segments_wire",
    "colsum_torch_order",
    "attention_ref64",
    "attention_bf16_staged",
]


def _abs_bits(x: torch.Tensor) -> torch.Tensor:
    """|x| as its int32 bit pattern: nonnegative floats order as integers."""
    return x.contiguous().view(torch.int32) & 0x7FFFFFFF


def _sel_gt(x: torch.Tensor, tau: float) -> torch.Tensor:
    """The selection rule of every thresholded op, as a bool mask: element i
    is selected iff bits(|x[i]|) > bits(float32(tau)) as unsigned integers;
    a float32(tau) below zero selects everything, +-0 included (-0.0 itself
    is not below zero and acts as 0).  NaN is therefore selected at every
    tau, inf at every finite tau, and subnormals compare exactly — the HIP
    kernels' sel_gt(abs_bits, tau_to_bits(tau)).  For NaN-free x and tau it
    is `x.abs() > tau`."""
    tb = torch.tensor(float(tau), dtype=torch.float64).to(torch.float32)
    if bool(tb < 0):
        return torch.ones(x.shape, dtype=torch.bool, device=x.device)
    return _abs_bits(x) > int(_abs_bits(tb.reshape(1)).item())


def kth_abs_value(t: torch.Tensor, k: int) -> float:
    """|t|'s k-th largest value (the exact top-k threshold).

    Reference: torch.topk in ratio2threshold, VGG/compression.py:370-381."""
    k = max(1, min(int(k), t.numel()))
    vals = torch.topk(t.abs().reshape(-1), k, sorted=True).values
    return float(vals[-1].item())


def compact_gt(t: torch.Tensor, tau: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Indices (int32, ascending) and values where |t| > tau (_sel_gt).

    Reference: compressbythreshold, VGG/compression.py:122-132."""
    flat = t.reshape(-1)
    idx = _sel_gt(flat, tau).nonzero(as_tuple=False).reshape(-1)
    return idx.to(torch.int32), flat[idx]


def count_gt(t: torch.Tensor, tau: float) -> int:
    return int(_sel_gt(t.reshape(-1), tau).sum().item())


def count_multi_gt(t: torch.Tensor, taus) -> list:
    flat = t.reshape(-1)
    return [int(_sel_gt(flat, float(x)).sum().item()) for x in taus]


def compact_adaptive(t: torch.Tensor, taus, hi_limit: int):
    """Adaptive-threshold compaction (fused in HIP): choose the first tau in
    `taus` whose selected count <= hi_limit (else the last), extract there.
    Returns (idx, val, chosen_index, chosen_count).  Mirrors the bump loop of
    add2residual, VGG/compression.py:384-404."""
    counts = count_multi_gt(t, taus)
    chosen = len(taus) - 1
    for c, tot in enumerate(counts):
        if c == len(taus) - 1 or tot <= hi_limit:
            chosen = c
            break
    idx, val = compact_gt(t, taus[chosen])
    return idx, val, chosen, counts[chosen]


def compact_adaptive_ef(t: torch.Tensor, residual: torch.Tensor, grad,
                        taus, hi_limit: int):
    """Torch oracle of the fused EF restore + adaptive compaction: restore
    (with optional bf16 grad upcast), snapshot residual, then the bump-rule
    compaction of compact_adaptive."""
    if grad is not None:
        restored = grad.reshape(-1).to(t.dtype) + residual
    else:
        restored = t + residual
    residual.copy_(restored)
    # t is deliberately NOT written (contract since round 2): the engine's
    # steady state densifies the result into t without reading the
    # restored values — saving a full-tensor write on the GPU path
    return compact_adaptive(restored, taus, hi_limit)


# every threshold the three-round refine loop of the gaussian compressors can
# visit, as multiples of tau0: level l, h high moves -> 0.5^(l-h) * 1.5^h at
# index l(l+1)/2 + h.  All factors are exact in binary.
GAUSS_FACTORS = (1.0, 0.5, 1.5, 0.25, 0.75, 2.25, 0.125, 0.375, 1.125, 3.375)


def gaussian_candidates(tau0: float) -> list:
    """cand[j] = float32(double(tau0) * F[j]), as Python floats."""
    t0 = float(torch.tensor(tau0, dtype=torch.float32))
    return [float(torch.tensor(t0 * f, dtype=torch.float64).to(torch.float32))
            for f in GAUSS_FACTORS]


def gaussian_tree_walk(counts, k: int) -> int:
    """Refine-tree walk over per-candidate counts (reference
    VGG/compression.py:236-255 in integers): 3*cnt < 2k -> low child,
    3*cnt > 4k -> high child, else stop; at most three counted rounds, the
    candidate reached after the third move is not re-tested."""
    l = h = 0
    for _ in range(3):
        cnt = int(counts[l * (l + 1) // 2 + h])
        if 3 * cnt < 2 * k:
            l += 1
        elif 3 * cnt > 4 * k:
            l += 1
            h += 1
        else:
            break
    return l * (l + 1) // 2 + h


def gaussian_select_ef(t: torch.Tensor, residual: torch.Tensor, grad,
                       density: float, k: int):
    """Torch oracle of the device-resident Gaussian-k selection: EF restore
    (with optional bf16 grad upcast) snapshotted into `residual` (t is NOT
    written, as in compact_adaptive_ef), Gaussian-fit threshold from fp64
    moments (reference utils.gen_threshold_from_normal_distribution,
    VGG/utils.py:136-138), the refine loop of VGG/compression.py:236-255
    over the float32 candidate table, and extraction at the chosen candidate.
    Returns (idx, val, chosen, count, tau, tau0, mean, std)."""
    import math

    if not (0.0 < density <= 1.0):
        raise ValueError("density must be in (0, 1]")
    if k < 1 or t.numel() < 1 or residual.numel() != t.numel():
        raise ValueError("gaussian_select_ef: bad k or sizes")
    if grad is not None:
        restored = grad.reshape(-1).to(t.dtype) + residual
    else:
        restored = t + residual
    residual.copy_(restored)
    v = restored.double()
    n = v.numel()
    mean = float(v.mean().item())
    std = float(v.std().item()) if n > 1 else 0.0
    if n < 2 or not math.isfinite(std) or std == 0.0:
        tau0d = abs(mean)
    else:
        z = float(torch.special.ndtri(
            torch.tensor(1.0 - density / 2.0, dtype=torch.float64)).item())
        tau0d = abs(mean + std * z)
    tau0 = float(torch.tensor(tau0d, dtype=torch.float64).to(torch.float32))
    cand = gaussian_candidates(tau0)
    counts = count_multi_gt(restored, cand)
    chosen = gaussian_tree_walk(counts, int(k))
    tau = cand[chosen]
    idx, val = compact_gt(restored, tau)
    return idx, val, chosen, counts[chosen], tau, tau0, mean, std


def topk_select(t: torch.Tensor, k: int):
    """Exact top-k by magnitude with a defined tie rule: the min(k, n)
    elements of largest |t| (compared on the abs bit pattern); with tau the
    k-th largest magnitude, everything above tau is taken and the tie class
    |t| == tau is filled from the lowest index up to exactly k.  Returns
    (idx int32 ascending, val, tau); writes nothing.

    Replaces torch.topk + gather in compress_org, VGG/compression.py:37-62."""
    flat = t.reshape(-1)
    n = flat.numel()
    if k < 1 or n < 1:
        raise ValueError("topk_select: k and n must be >= 1")
    k = min(int(k), n)
    bits = _abs_bits(flat)
    tau_bits = torch.kthvalue(bits, n - k + 1).values
    gt = bits > tau_bits
    eq = bits == tau_bits
    need = k - int(gt.sum().item())
    sel = gt | (eq & (torch.cumsum(eq, 0) <= need))
    idx = sel.nonzero(as_tuple=False).reshape(-1)
    tau = float(tau_bits.reshape(1).view(torch.float32).item())
    return idx.to(torch.int32), flat[idx], tau


def topk_select_ef(t: torch.Tensor, residual: torch.Tensor, grad, k: int):
    """topk_select over restored = float(grad) + residual (grad bf16) or
    t + residual, with the compress_org residual update fused in: on return
    residual holds restored with +0.0 at the selected positions.  t is NOT
    written (as in gaussian_select_ef).  Returns (idx, val, tau)."""
    if residual.numel() != t.numel():
        raise ValueError("topk_select_ef: residual size mismatch")
    if grad is not None:
        restored = grad.reshape(-1).to(t.dtype) + residual
    else:
        restored = t.reshape(-1) + residual
    idx, val, tau = topk_select(restored, k)
    residual.copy_(restored)
    residual[idx.long()] = 0.0
    return idx, val, tau


def sparse_merge_topk(a_idx: torch.Tensor, a_val: torch.Tensor,
                      b_idx: torch.Tensor, b_val: torch.Tensor, k: int):
    """Top-k of the sum of two sparse vectors (ascending unique int32
    indices) without densifying: the union over indices, a_val + b_val where
    both hold an index (a sum of exactly 0 stays in the union), truncated to
    the min(k, |union|) largest |v| with topk_select's lowest-index tie
    rule.  Returns (idx ascending, val).

    Replaces the zeros(n) + two scatters + torch.topk of the gTopK tree
    merge, VGG/allreducer.py:116-150."""
    if k < 1:
        raise ValueError("sparse_merge_topk: k must be >= 1")
    idx = torch.cat([a_idx, b_idx])
    val = torch.cat([a_val, b_val])
    m = idx.numel()
    if m == 0:
        return idx, val
    order = torch.argsort(idx, stable=True)  # a before b where equal
    si, sv = idx[order], val[order]
    first = torch.ones(m, dtype=torch.bool, device=idx.device)
    first[1:] = si[1:] != si[:-1]
    has_twin = torch.zeros_like(first)
    has_twin[:-1] = ~first[1:]
    summed = torch.where(has_twin, sv + torch.roll(sv, -1), sv)
    u_idx, u_val = si[first], summed[first]
    pos, out_val, _ = topk_select(u_val, k)
    return u_idx[pos.long()], out_val


def scatter_add_(dest: torch.Tensor, idx: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    """dest[idx] += val (duplicate indices accumulate).

    Reference: reduced_t[indexes] += values, VGG/allreducer.py:779,794."""
    dest.reshape(-1).index_add_(0, idx.long(), val.to(dest.dtype))
    return dest


def zero_at_(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """t[idx] = 0. Reference: update_residuals, VGG/compression.py:467-471."""
    t.reshape(-1)[idx.long()] = 0
    return t


def zero_at_masked_(t: torch.Tensor, idx: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """t[idx[i]] = 0 wherever mask[idx[i]] (fused residual credit)."""
    j = idx.long()
    sel = j[mask[j]]
    t.reshape(-1)[sel] = 0
    return t


def fill_sparse_scaled_(
    out: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, scale: float
) -> torch.Tensor:
    """out.zero_(); out[idx] = val * scale.

    Reference: result.fill_(0); result[idx] = values/P, VGG/allreducer.py:838-841."""
    flat = out.reshape(-1)
    flat.zero_()
    flat[idx.long()] = val.to(flat.dtype) * scale
    return out


def isin_sorted(a: torch.Tensor, b_sorted: torch.Tensor) -> torch.Tensor:
    """Boolean mask: which elements of a are present in ascending-sorted b.

    Reference: np.intersect1d for residual credit, VGG/allreducer.py:844,1051
    (BERT uses the same searchsorted trick, BERT/bert/allreducer.py:21-24)."""
    if b_sorted.numel() == 0:
        return torch.zeros(a.numel(), dtype=torch.bool, device=a.device)
    a64 = a.long()
    b64 = b_sorted.long()
    pos = torch.searchsorted(b64, a64).clamp_(max=b64.numel() - 1)
    return b64[pos] == a64


def ef_restore_upcast_(t: torch.Tensor, residual: torch.Tensor,
                       g: torch.Tensor) -> torch.Tensor:
    """t = float(g) + residual; residual = t (fused upcast + EF restore)."""
    t.copy_(g.to(t.dtype))
    t.add_(residual)
    residual.copy_(t)
    return t


def ef_restore_snapshot_(t: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """t += residual; residual = t  (fused in HIP).

    Reference: ratio2threshold / add2residual preamble,
    VGG/compression.py:375-379,389-391."""
    t.add_(residual)
    residual.copy_(t)
    return t


def fused_sgd_(
    param: torch.Tensor,
    grad: torch.Tensor,
    momentum_buf: torch.Tensor,
    lr: float,
    momentum: float,
    weight_decay: float,
    nesterov: bool,
) -> None:
    """SGD with momentum/nesterov/weight-decay.

    Reference: _DistributedOptimizer._step, VGG/distributed_optimizer.py:107-145."""
    d_p = grad
    if weight_decay != 0:
        d_p = d_p.add(param, alpha=weight_decay)
    if momentum != 0:
        momentum_buf.mul_(momentum).add_(d_p)
        d_p = d_p.add(momentum_buf, alpha=momentum) if nesterov else momentum_buf
    param.add_(d_p, alpha=-lr)


def fused_adam_(
    param: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    gscale=None,
) -> None:
    """BertAdam-style update: no bias correction, decoupled weight decay.
    `gscale` (1-elem tensor) pre-scales the gradient read (device clip).

    Reference: BertAdam.step, BERT/bert/transformers/optimization.py:183-224."""
    if gscale is not None:
        grad = grad * gscale.to(grad.device, grad.dtype)
    exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    update = exp_avg / (exp_avg_sq.sqrt() + eps)
    if weight_decay != 0:
        update = update + weight_decay * param
    param.add_(update, alpha=-lr)


# -- dense Adam: fp64 oracle and rounding bounds ------------------------------
# The HIP kernel (adam_one in ops/csrc/kernels.hip) receives every
# hyperparameter as an fp32 scalar and forms 1 - b in fp32:
#
#     gi = g*gs                         (gs = *gscale, 1 without one)
#     m' = m*b1 + c1*gi                 c1 = fp32(1 - b1)
#     v' = v*b2 + (c2*gi)*gi            c2 = fp32(1 - b2)
#     p' = p - lr*(m'/(sqrt(v') + eps) + wd*p)
#
# adam_ref64 is that formula in fp64 over the same fp32 inputs and the same
# fp32 hyperparameters.  fused_adam_ above follows torch's convention instead
# (Python doubles, 1 - b as a double): at b2 = 0.999 its 1 - b2 differs from
# the kernel's c2 by 1.3e-5 relative, dozens of times the rounding bound on
# v (tests/test_core_kernels_reference.py measures it).

ADAM_U = 2.0 ** -24       # fp32 unit roundoff
ADAM_TINY = 2.0 ** -149   # smallest fp32 subnormal: absolute slack


def _f32(x) -> float:
    return float(torch.tensor(float(x), dtype=torch.float64).to(torch.float32))


def adam_hyper_f32(lr, b1, b2, eps, wd, gscale=None):
    """(lr, b1, b2, eps, wd, gs, c1, c2) as the kernel sees them: each
    rounded to fp32, c = fp32(1 - b) from the rounded b, gs = 1 without a
    gscale.  Python floats holding fp32 values."""
    lr, b1, b2, eps, wd = (_f32(x) for x in (lr, b1, b2, eps, wd))
    gs = 1.0 if gscale is None else _f32(
        gscale.item() if torch.is_tensor(gscale) else gscale)
    return lr, b1, b2, eps, wd, gs, _f32(1.0 - b1), _f32(1.0 - b2)


def adam_ref64(p, g, m, v, lr, b1, b2, eps, wd, gscale=None):
    """One Adam step in fp64 on the fp32 inputs, under the kernel's
    hyperparameter convention.  Writes nothing.  Returns (m64, v64, p_of):
    the new moments, and a function p_of(m_new, v_new) -> p64 that takes the
    step from any pair of moments — fed the kernel's own stored m', v', the
    p check is not charged with the moments' error."""
    lr, b1, b2, eps, wd, gs, c1, c2 = adam_hyper_f32(lr, b1, b2, eps, wd,
                                                     gscale)
    p64, g64 = p.double(), g.double() * gs
    m64 = m.double() * b1 + c1 * g64
    v64 = v.double() * b2 + c2 * g64 * g64

    def p_of(m_new, v_new):
        up = m_new.double() / (v_new.double().sqrt() + eps) + wd * p64
        return p64 - lr * up

    return m64, v64, p_of


def adam_bounds(p, g, m, v, m_new, v_new, lr, b1, b2, eps, wd, gscale=None):
    """Elementwise bounds (bm, bv, bp), fp64, on |m' - m64|, |v' - v64| and
    |p' - p_of(m', v')| for a correct fp32 evaluation of the formula above,
    with u = 2^-24.  Each factor is the number of fp32 roundings on the
    term's path plus one of slack (which also covers the u^2 terms):

      bm = 4u(|m*b1| + |c1*g*gs|)   g*gs, c1*gi and the sum: 3 roundings on
                                    the gradient term, 2 on the state term
      bv = 6u*v64                   g*gs counted twice, c2*gi, *gi, the sum:
                                    5; every term is non-negative
      bp = u|p64| + 6u*lr(|m'/(sqrt(v') + eps)| + |wd*p|)
                                    sqrt, + eps, the division, + wd*p and
                                    lr*up: 5, and u|p64| for the final
                                    subtraction

    plus ADAM_TINY (one fp32 subnormal) each, for results that underflow.
    A fused multiply-add only removes a rounding.  Correctly rounded fp32
    sqrt and division are assumed (the compiler's default; the build passes
    no fast-math flag).  m_new, v_new are the moments p' was computed from."""
    lr, b1, b2, eps, wd, gs, c1, c2 = adam_hyper_f32(lr, b1, b2, eps, wd,
                                                     gscale)
    u = ADAM_U
    p64, g64 = p.double(), g.double() * gs
    _, v64, p_of = adam_ref64(p, g, m, v, lr, b1, b2, eps, wd, gs)
    bm = 4 * u * ((m.double() * b1).abs() + (c1 * g64).abs()) + ADAM_TINY
    bv = 6 * u * v64 + ADAM_TINY
    step = (m_new.double() / (v_new.double().sqrt() + eps)).abs()
    bp = (u * p_of(m_new, v_new).abs()
          + 6 * u * lr * (step + (wd * p64).abs()) + ADAM_TINY)
    return bm, bv, bp


def scatter_gt_credit_(result, residual, idx, val, tau, scale=1.0) -> int:
    sel = _sel_gt(val, tau)
    j = idx.long()[sel]
    result[j] = val[sel] * scale
    residual[j] = 0.0
    return int(sel.sum())


def credit_gt_(residual, idx, val, tau) -> int:
    """scatter_gt_credit_ without the dense result: residual[idx] = 0 where
    |val| > tau; returns the count."""
    sel = _sel_gt(val, tau)
    residual[idx.long()[sel]] = 0.0
    return int(sel.sum())


# -- sparse optimizer tail --------------------------------------------------
# A sparse gradient (idx int32 ascending+unique, val fp32, scale, tau) stands
# for the dense vector that is val[i]*scale at idx[i] where |val[i]| > tau
# (tau < 0 keeps every entry) and +0.0 elsewhere.

def _sparse_kept(val: torch.Tensor, tau: float) -> torch.Tensor:
    return _sel_gt(val, tau)


def densify_sparse_grad(idx, val, base: int, n: int, scale: float, tau: float):
    """The slice [base, base+n) of the dense gradient a sparse one stands
    for, as a fresh fp32 tensor."""
    g = torch.zeros(n, dtype=torch.float32, device=val.device)
    j = idx.long() - int(base)
    keep = _sparse_kept(val, tau) & (j >= 0) & (j < n)
    g[j[keep]] = val[keep] * scale
    return g


def sparse_sumsq_into_(acc: torch.Tensor, idx, val, scale: float,
                       tau: float) -> None:
    """acc (fp64[1]) += sum of squares of the dense gradient: the kept
    val*scale products, rounded to fp32 as the scatter stores them."""
    g = val[_sparse_kept(val, tau)] * scale
    acc += (g.double() ** 2).sum()


def grad_clip_scale_sparse(idx, val, scale: float, tau: float,
                           max_norm: float, n: int) -> torch.Tensor:
    """grad_clip_scale of the length-n dense gradient.  Densifies, so the
    norm is summed in exactly the dense route's order and the two routes
    agree to the bit (the HIP op sums the kept entries only and ignores n)."""
    return grad_clip_scale(densify_sparse_grad(idx, val, 0, n, scale, tau),
                           max_norm)


def fused_adam_sparse_(param, idx, val, base, scale, tau, exp_avg, exp_avg_sq,
                       lr, beta1, beta2, eps, weight_decay, gscale=None) -> None:
    """fused_adam_ with the gradient slice [base, base+len(param)) given in
    sparse form: densify into a temporary, then the dense update."""
    g = densify_sparse_grad(idx, val, base, param.numel(), scale, tau)
    fused_adam_(param, g, exp_avg, exp_avg_sq, lr, beta1, beta2, eps,
                weight_decay, gscale)


# -- flat SGD -----------------------------------------------------------------

def sgd_step_(param, grad, momentum_buf, lr, momentum, weight_decay, nesterov,
              gscale=None) -> None:
    """SGD step with momentum / nesterov / weight decay (no dampening), every
    multiply and add a separate fp32 rounding, in the HIP kernel's order:

        gi = g*gs            (only when gscale is given)
        d  = gi + wd*p       (skipped when wd == 0)
        b  = buf*mom + d;  buf = b
        d  = nesterov ? d + mom*b : b
        p  = p - lr*d

    Separate mul / add calls and no `alpha=` (which may fuse), so the result
    has the same bits on any device for finite, non-subnormal data.
    `momentum_buf` is not touched when momentum == 0."""
    def f32(x):  # the kernel's scalar arguments are fp32
        return float(torch.tensor(float(x), dtype=torch.float32))

    lr, momentum, weight_decay = f32(lr), f32(momentum), f32(weight_decay)
    d = grad
    if gscale is not None:
        d = d * gscale.to(grad.device, grad.dtype)
    if weight_decay != 0:
        d = d + param * weight_decay
    if momentum != 0:
        momentum_buf.mul_(momentum)
        momentum_buf.add_(d)
        d = d + momentum_buf * momentum if nesterov else momentum_buf
    param.sub_(d * lr)


def sgd_step_sparse_(param, idx, val, base, scale, tau, momentum_buf, lr,
                     momentum, weight_decay, nesterov, gscale=None) -> None:
    """sgd_step_ with the gradient slice [base, base+len(param)) given in
    sparse form: densify into a temporary, then the dense update."""
    g = densify_sparse_grad(idx, val, base, param.numel(), scale, tau)
    sgd_step_(param, g, momentum_buf, lr, momentum, weight_decay, nesterov,
              gscale)


def clip_scale_from_sumsq(acc: torch.Tensor, max_norm: float) -> torch.Tensor:
    """The clip factor from an fp64 sum of squares, as the HIP clip-scale
    kernel computes it: gn = sqrt(acc); gn > max ? fp32(max / (gn + 1e-6))
    : 1, with max rounded to fp32 first.  A 1-elem fp32 tensor."""
    gn = acc.reshape(1).sqrt()
    mx = torch.full_like(gn, float(torch.tensor(float(max_norm),
                                                dtype=torch.float32)))
    # tensor / tensor: a true division (scalar / tensor is reciprocal * scalar)
    return torch.where(gn > mx, mx / (gn + 1e-6),
                       torch.ones_like(gn)).to(torch.float32)


# -- sparse wire codec ------------------------------------------------------
# Wire layout (AllReducer._pack / _unpack / _pack_ints): segment j with c_j
# elements is c_j int32 indices followed by the values — c_j fp32 words, or
# ceil(c_j/2) int32 words of bf16 with a ZERO trailing half-word when c_j is
# odd.  Segments are concatenated in destination / rank order.

def _wire_words(c: int, wire_bf16: bool) -> int:
    return c + (c + 1) // 2 if wire_bf16 else 2 * c


def pack_regions(idx: torch.Tensor, val: torch.Tensor, bounds: torch.Tensor,
                 wire_bf16: bool):
    """Split the ascending selection (idx int32, val fp32) at the int64
    [P+1] CPU boundary table and pack it: segment j holds the elements with
    bounds[j] <= idx < bounds[j+1] (lower-bound rule — an index equal to a
    boundary goes to the upper region).  Returns (buf int32, counts list).

    Reference: the per-destination send buffers of the round-1 exchange,
    VGG/allreducer.py:682-693."""
    P = bounds.numel() - 1
    m = idx.numel()
    cuts = [0, m]
    if P > 1:
        split = torch.searchsorted(idx.long(), bounds[1:P].to(idx.device)).cpu()
        cuts = [0] + [int(x) for x in split] + [m]
    counts = [cuts[j + 1] - cuts[j] for j in range(P)]
    segs = []
    for j in range(P):
        i, v = idx[cuts[j]:cuts[j + 1]], val[cuts[j]:cuts[j + 1]]
        if wire_bf16:
            v = v.to(torch.bfloat16)
            if v.numel() % 2:
                v = torch.cat([v, v.new_zeros(1)])
        segs += [i.view(torch.int32), v.view(torch.int32)]
    return torch.cat(segs), counts


def unpack_segments(buf: torch.Tensor, counts, wire_bf16: bool):
    """Gather rank-ordered wire segments into contiguous (idx int32, val
    fp32); `counts` are ELEMENT counts per segment."""
    idxs, vals = [], []
    off = 0
    for n in counts:
        ints = _wire_words(n, wire_bf16)
        idxs.append(buf[off:off + n])
        if wire_bf16:
            vals.append(buf[off + n:off + ints].view(torch.bfloat16)[:n].float())
        else:
            vals.append(buf[off + n:off + ints].view(torch.float32))
        off += ints
    if not idxs:
        return buf[:0], buf[:0].view(torch.float32)
    return torch.cat(idxs), torch.cat(vals)


def unpack_scatter_add_(dest: torch.Tensor, buf: torch.Tensor, counts,
                        base: int, wire_bf16: bool) -> torch.Tensor:
    """dest[idx - base] += val over every wire entry (fused in HIP, which
    never materialises idx / val).  The caller guarantees
    base <= idx < base + dest.numel().

    Reference: reduced_t[indexes - offset] += values, VGG/allreducer.py:779,794."""
    idx, val = unpack_segments(buf, counts, wire_bf16)
    if idx.numel():
        scatter_add_(dest, idx - int(base), val)
    return dest


def round2_tail_(residual: torch.Tensor, idx: torch.Tensor,
                 all_idx: torch.Tensor, all_val: torch.Tensor, k=None):
    """Ok-Topk round-2 tail over the gathered survivors (all_idx int32
    ascending and unique, all_val fp32) and this rank's local selection idx
    (int32 ascending, unique): the global selection plus the residual
    credit.  Returns (g_idx, g_val, tau).

    k is None (threshold iteration) or no entry was gathered: the selection
    is every gathered entry, returned as passed in; tau is None.  k given:
    the min(k, S) entries of largest |all_val| by topk_select's rule (abs
    bit pattern, the tie class at the k-th magnitude filled from the lowest
    position), g_idx ascending, tau the k-th magnitude.

    Credit: residual[j] = +0.0 for every j in both g_idx and idx, and no
    other write; a matched j outside [0, residual.numel()) is dropped.

    Reference: k2globalthreshold + gather and intersect1d +
    update_residuals, VGG/allreducer.py:833-845,1051-1052."""
    if k is not None and k < 1:
        raise ValueError("round2_tail_: k must be >= 1")
    if all_idx.numel() != all_val.numel():
        raise ValueError("round2_tail_: all_idx / all_val length mismatch")
    if k is None or all_idx.numel() == 0:
        g_idx, g_val, tau = all_idx, all_val, None
    else:
        pos, g_val, tau = topk_select(all_val, k)
        g_idx = all_idx[pos.long()]
    if idx.numel() and g_idx.numel():
        hit = g_idx[isin_sorted(g_idx, idx)].long()
        hit = hit[(hit >= 0) & (hit < residual.numel())]
        residual.reshape(-1)[hit] = 0.0
    return g_idx, g_val, tau


def round2_tail_wire_(residual: torch.Tensor, idx: torch.Tensor,
                      buf: torch.Tensor, counts, wire_bf16: bool, k=None):
    """round2_tail_ with the gathered survivors given as the allgathered
    wire buffer (`counts` are ELEMENT counts per rank segment): bit-equal to
    round2_tail_ over unpack_segments(buf, counts, wire_bf16), which with
    k=None is also the returned pair."""
    all_idx, all_val = unpack_segments(buf, counts, wire_bf16)
    return round2_tail_(residual, idx, all_idx, all_val, k)


# -- Ok-Topk round-1 reduce at a region owner --------------------------------

def reduce_segments(idx: torch.Tensor, val: torch.Tensor, counts, base: int,
                    length: int, tau: float):
    """Reduce of the payload a region owner receives in round 1: `idx`
    (int32) / `val` (fp32) hold len(counts) concatenated segments in rank
    order, segment j with counts[j] entries, ascending and duplicate-free.

    This composition is the definition.  Start from `length` zeros; for
    every entry with base <= idx < base + length add val at idx - base,
    segments in order and entries within a segment in order, each add one
    fp32 add (entries outside the range are dropped); keep the positions
    with |sum| > tau as a float comparison (exact cancellations and NaN
    sums go at tau = 0 — for NaN not compact_gt's bit rule, which keeps it;
    the HIP reduce tests fabsf(s) > tau) and return them ascending as
    (g_idx = position + base int32, g_val = sum fp32).  tau >= 0.

    Reference: reduced_t[indexes - offset] += values over the rank-ordered
    receive buffers, then compressbythreshold, VGG/allreducer.py:779,794,894."""
    if tau < 0:
        raise ValueError("reduce_segments: tau must be >= 0")
    if length < 0:
        raise ValueError("reduce_segments: length must be >= 0")
    if idx.numel() != val.numel() or sum(counts) != idx.numel():
        raise ValueError("reduce_segments: idx / val / counts length mismatch")
    reduced = torch.zeros(int(length), dtype=torch.float32, device=val.device)
    d = idx.long() - int(base)
    inside = (d >= 0) & (d < int(length))
    if bool(inside.any()):
        reduced.index_add_(0, d[inside], val[inside])
    keep = (reduced.abs() > float(tau)).nonzero(as_tuple=False).reshape(-1)
    return keep.to(torch.int32) + int(base), reduced[keep]


def reduce_segments_wire(buf: torch.Tensor, counts, wire_bf16: bool, base: int,
                         length: int, tau: float):
    """reduce_segments with the segments still packed in the wire layout
    (`counts` are ELEMENT counts per segment): bit-equal to reduce_segments
    over unpack_segments(buf, counts, wire_bf16)."""
    idx, val = unpack_segments(buf, counts, wire_bf16)
    return reduce_segments(idx, val, counts, base, length, tau)


def grad_clip_scale(t: torch.Tensor, max_norm: float) -> torch.Tensor:
    gn = t.reshape(-1).float().norm(p=2)
    scale = torch.where(gn > max_norm, max_norm / (gn + 1e-6),
                        torch.ones_like(gn))
    return scale.reshape(1)


def sumsq_into_(acc: torch.Tensor, t: torch.Tensor) -> None:
    acc += (t.reshape(-1).double() ** 2).sum()


def l2norm(t: torch.Tensor) -> float:
    return float(t.reshape(-1).norm(p=2).item())


def colsum_torch_order(x: torch.Tensor, bh: int = 2, ctas: int = 32,
                       vt0: int = 4) -> torch.Tensor:
    """fp32 column sum of x [R, C] in the order torch's GPU reduction
    (ATen/native/cuda/Reduce.cuh, reduce over the slow dimension) adds it:
    the association tree native colsum_bf16_into_exact reproduces.

    bh: block height, ctas: blocks per output, vt0: accumulators per thread.
    Defaults are torch's configuration for bf16 [1024, 768 | 2304 | 3072] on
    a 256-CU device; bh = 1, ctas = 1 stands for "rows not split over
    threadIdx.y".  All adds are plain fp32, every accumulator starts at +0:
      * lane l = ty + by*bh (ty < bh, by < ctas) takes rows l, l + bh*ctas,
        ...; its k-th row goes to accumulator k mod vt0;
      * T(l) = ((A0 + A1) + A2) + ... ;
      * P(by): tree over ty, T[ty] += T[ty + off] for off = bh/2 ... 1;
      * ctas > 1: G(ty) = ((0 + P(ty)) + P(ty + bh)) + ..., then the same
        tree over G.
    Returns the fp32 sum; the kernel rounds it once to bf16."""
    assert x.dim() == 2 and bh >= 1 and ctas >= 1 and vt0 >= 1
    assert bh & (bh - 1) == 0, "bh is a power of two"
    xf = x.detach().float().cpu()
    R, C = xf.shape
    zero = torch.zeros(C, dtype=torch.float32)
    step = bh * ctas

    def tree(vals):
        vals = list(vals)
        off = len(vals) // 2
        while off > 0:
            for ty in range(off):
                vals[ty] = vals[ty] + vals[ty + off]
            off //= 2
        return vals[0]

    T = []
    for lane in range(step):
        acc = [zero.clone() for _ in range(vt0)]
        for k, r in enumerate(range(lane, R, step)):
            acc[k % vt0] = acc[k % vt0] + xf[r]
        t = acc[0]
        for a in acc[1:]:
            t = t + a
        T.append(t)
    P = [tree(T[by * bh:(by + 1) * bh]) for by in range(ctas)]
    if ctas == 1:
        return P[0]
    G = []
    for ty in range(bh):
        g = zero.clone()
        for j in range(ty, ctas, bh):
            g = g + P[j]
        G.append(g)
    return tree(G)


# -- flash attention --------------------------------------------------------
# Two references of the op of ops/csrc/attention_fa.hip over the packed bf16
# projection buffer qkv [b, s, 3*nh*64]: ctx = (softmax(QK^T/8 + mask) *
# keep) @ V, and its gradient for an upstream gy [b, s, nh*64].  mask is
# additive over keys ([b, s] or anything that reshapes to it; rounded to
# bf16 as the binding does) or None; keep is [b*nh, s, s] holding
# 1/keep_prob where the dropout kept an entry and 0 where it dropped it, or
# None.  Both return AttnRef(out [b, s, nh*64], lse [b*nh, s],
# dqkv [b, s, 3*nh*64]) in their working precision.

AttnRef = collections.namedtuple("AttnRef", ["out", "lse", "dqkv"])

ATTN_HD = 64


def attn_split_heads(qkv: torch.Tensor, num_heads: int):
    """q, k, v as [b, nh, s, 64] views of the packed [b, s, 3*nh*64]."""
    b, s, _ = qkv.shape
    return qkv.reshape(b, s, 3, num_heads, ATTN_HD).permute(2, 0, 3, 1, 4).unbind(0)


def attn_merge_heads(x: torch.Tensor) -> torch.Tensor:
    """[b, nh, s, 64] -> [b, s, nh*64]."""
    b, nh, s, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, s, nh * hd)


def _attn_mask_keep(qkv, mask, keep, num_heads, dtype):
    b, s, _ = qkv.shape
    m = None
    if mask is not None and mask.numel():
        m = mask.reshape(b, 1, 1, s).to(torch.bfloat16).to(dtype)
    kp = None
    if keep is not None:
        kp = keep.reshape(b, num_heads, s, s).to(dtype)
    return m, kp


def _bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def attention_ref64(qkv, mask, gy, num_heads, keep=None) -> AttnRef:
    """The operation in fp64 from the same bf16 inputs; the gradient is
    autograd's, in fp64.  This is the oracle."""
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = attn_split_heads(x, num_heads)
    m, kp = _attn_mask_keep(qkv, mask, keep, num_heads, torch.float64)
    sc = q @ k.transpose(-1, -2) / math.sqrt(ATTN_HD)
    if m is not None:
        sc = sc + m
    lse = torch.logsumexp(sc, dim=-1)
    p = torch.softmax(sc, dim=-1)
    if kp is not None:
        p = p * kp
    out = attn_merge_heads(p @ v)
    (dqkv,) = torch.autograd.grad(out, x, gy.detach().double())
    b, s, _ = qkv.shape
    return AttnRef(out.detach(), lse.detach().reshape(b * num_heads, s), dqkv)


# attention_bf16_staged is built from the steps below so that each can be
# driven on its own (the CPU tests feed them deliberately wrong arguments).
# All of them work in fp32 on whole rows (no tiling) over [b, nh, s, *]
# tensors and round to bf16 exactly where the kernels do.

def attn_staged_inputs(qkv, mask, gy, num_heads, keep=None):
    """(q, k, v, go [b, nh, s, 64], mask [b, 1, 1, s] | None,
    keep [b, nh, s, s] | None, scale), all fp32."""
    b, s, _ = qkv.shape
    q, k, v = attn_split_heads(qkv.detach().float(), num_heads)
    m, kp = _attn_mask_keep(qkv, mask, keep, num_heads, torch.float32)
    go = gy.detach().float().reshape(b, s, num_heads, ATTN_HD).permute(0, 2, 1, 3)
    return q, k, v, go, m, kp, 1.0 / math.sqrt(ATTN_HD)


def attn_staged_result(o, lse, dq, dk, dv) -> AttnRef:
    b, nh, s, _ = o.shape
    return AttnRef(attn_merge_heads(o), lse.reshape(b * nh, s),
                   attn_pack_grads(dq, dk, dv))


def attn_staged_scores(q, k, mask, scale):
    """s = (q.k)*scale + mask, fp32."""
    sc = (q @ k.transpose(-1, -2)) * scale
    return sc if mask is None else sc + mask


def attn_staged_forward(q, k, v, mask, keep, scale):
    """attn_fwd_fa_kernel: m = rowmax, e = exp(s - m), l = sum(e) (before
    dropout, from the unrounded e), P~ = bf16(e*keep), O = bf16((P~ @ V)/l),
    lse = m + log(l).  Returns (O bf16-rounded, lse, O before rounding)."""
    sc = attn_staged_scores(q, k, mask, scale)
    m = sc.amax(dim=-1, keepdim=True)
    e = torch.exp(sc - m)
    l = e.sum(dim=-1, keepdim=True)
    pt = _bf16_round(e if keep is None else e * keep)
    o32 = (pt @ v) / l
    return _bf16_round(o32), (m + torch.log(l)).squeeze(-1), o32


def attn_staged_p(q, k, lse, mask, scale):
    """The backward's recomputed P = exp(s - lse), fp32, not rounded."""
    return torch.exp(attn_staged_scores(q, k, mask, scale) - lse.unsqueeze(-1))


def attn_staged_ds(p, go, v, dvec, keep, scale):
    """dP = (gO @ V^T)*keep, dS = bf16(p*(dP - D)*scale)."""
    dp = go @ v.transpose(-1, -2)
    if keep is not None:
        dp = dp * keep
    return _bf16_round(p * (dp - dvec.unsqueeze(-1)) * scale)


def attn_staged_dq(ds, k):
    return _bf16_round(ds @ k)


def attn_staged_dk(ds, q):
    return _bf16_round(ds.transpose(-1, -2) @ q)


def attn_staged_dv(p, go, keep):
    a = _bf16_round(p if keep is None else p * keep)
    return _bf16_round(a.transpose(-1, -2) @ go)


def attn_pack_grads(dq, dk, dv) -> torch.Tensor:
    """[b, nh, s, 64] x 3 -> packed [b, s, 3*nh*64]."""
    b, nh, s, hd = dq.shape
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(
        b, s, 3 * nh * hd)


def attention_bf16_staged(qkv, mask, gy, num_heads, keep=None) -> AttnRef:
    """The same mathematics in fp32 with a bf16 rounding at exactly the
    points where the kernels of attention_fa.hip round.  NOT an oracle: its
    distance from attention_ref64 is what the kernels' chosen precision
    costs when everything else is right — the yardstick the accuracy tests
    scale their bounds by.  Left out on purpose: __expf/__logf, the MFMA
    accumulation order and the fp32 reorderings of the online rescale."""
    q, k, v, go, m, kp, scale = attn_staged_inputs(qkv, mask, gy, num_heads, keep)
    o, lse, _ = attn_staged_forward(q, k, v, m, kp, scale)
    dvec = (go * o).sum(dim=-1)  # attn_rowdot, from the bf16 O
    p = attn_staged_p(q, k, lse, m, scale)
    ds = attn_staged_ds(p, go, v, dvec, kp, scale)
    return attn_staged_result(o, lse, attn_staged_dq(ds, k),
                              attn_staged_dk(ds, q), attn_staged_dv(p, go, kp))


# Accuracy metrics of the attention tests.  Each tensor is viewed as rows of
# 64 (one head's vector at one position); both metrics are relative to the
# fp64 reference.

def attn_tensors(res: AttnRef, num_heads: int) -> dict:
    """out, dq, dk, dv as [rows, 64] fp64, rows indexed (b, position, head)."""
    b, s, _ = res.out.shape
    g = res.dqkv.reshape(b, s, 3, num_heads, ATTN_HD).double()
    return {"out": res.out.double().reshape(-1, ATTN_HD),
            "dq": g[:, :, 0].reshape(-1, ATTN_HD),
            "dk": g[:, :, 1].reshape(-1, ATTN_HD),
            "dv": g[:, :, 2].reshape(-1, ATTN_HD)}


def attn_rel_fro(x: torch.Tensor, ref: torch.Tensor) -> float:
    """||x - ref||_F / ||ref||_F."""
    return float((x - ref).norm() / ref.norm())


def attn_row_max(x: torch.Tensor, ref: torch.Tensor) -> float:
    """max over rows ||x_row - ref_row||_2 / median over rows ||ref_row||_2,
    so that one wrong row is not diluted by the rest of the tensor.  Where
    more than half of the reference rows are exactly zero (dK and dV rows of
    keys whose mask underflows the softmax) the median is taken over the
    nonzero rows: the denominator only sets the unit, and cancels whenever
    two results are compared against the same reference."""
    norms = ref.norm(dim=1)
    med = norms.median()
    if float(med) == 0.0:
        med = norms[norms > 0].median()
    return float((x - ref).norm(dim=1).max() / med)


# A kernel result passes when each metric, per tensor, is at most this many
# times the same metric of attention_bf16_staged on the same inputs.  The
# staged reference carries every bf16 rounding the kernels make; the factor
# covers what it leaves out on purpose — __expf/__logf, the MFMA
# accumulation order and the fp32 reorderings of the online rescale.  The
# staged reference sits at rel_fro 0.0023-0.0036, while the smallest error
# worth catching, 2 % in `scale` on the dS path, lifts dQ/dK to 0.020 (8.5x
# the floor) and one duplicated dQ row gives row_max >= 1: 3x leaves room
# for the kernel and still catches both.  If a case exceeds it the kernel
# is wrong or rounds where the emulation does not; the factor is not tuned.
ATTN_STAGED_FACTOR = 3.0


def attn_metrics(res: AttnRef, ref64: AttnRef, num_heads: int) -> dict:
    """{tensor: (rel_fro, row_max)} of res against the fp64 reference."""
    x, r = attn_tensors(res, num_heads), attn_tensors(ref64, num_heads)
    return {n: (attn_rel_fro(x[n], r[n]), attn_row_max(x[n], r[n])) for n in r}


def attn_over_staged(metrics: dict, staged: dict, names=None) -> list:
    """The (tensor, metric) pairs of `metrics` that exceed
    ATTN_STAGED_FACTOR times the staged reference's."""
    bad = []
    for n in (names or metrics):
        for i, what in enumerate(("rel_fro", "row_max")):
            if not metrics[n][i] <= ATTN_STAGED_FACTOR * staged[n][i]:
                bad.append((n, what))
    return bad


def attn_lse_bound(lse64: torch.Tensor) -> torch.Tensor:
    """Elementwise bound on |lse - lse64|: max(2^-10, 2*ulp_fp32(|lse64|)).
    2^-10 keeps the relative error an LSE error induces in every recomputed
    P below half a bf16 ulp, the precision P is staged at; the ulp term
    only matters where |lse| ~ 1e4 (a fully masked batch)."""
    a = lse64.abs().float()
    ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
    return torch.clamp(2.0 * ulp, min=2.0 ** -10)
