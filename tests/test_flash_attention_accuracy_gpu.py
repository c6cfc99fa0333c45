"""Flash attention (ops/csrc/attention_fa.hip) against an fp64 reference,
per tensor.

Every case runs forward and backward through _FlashAttention.apply, so
attn_fwd_fa_kernel, attn_rowdot, attn_bwd_dq_kernel and attn_bwd_dkv_kernel
are all exercised, and checks out, lse, dQ, dK and dV separately:

  * out, dQ, dK, dV: rel_fro and row_max against R.attention_ref64 must each
    be at most R.ATTN_STAGED_FACTOR times what R.attention_bf16_staged — the
    same mathematics with the kernels' bf16 roundings and nothing else —
    scores on the same inputs.  No absolute constant.
  * lse: |lse - lse64| <= R.attn_lse_bound (derived, see there).

tests/test_flash_attention_reference.py shows on the CPU that these criteria
reject a set of subtly wrong backwards.  Each check prints its figures
(pytest -s) before it asserts; profiles/README.md holds a recorded table."""
import pytest
import torch

from attn_cases import REGIMES, make_case
from oktopk_amd.ops import reference as R

pytestmark = pytest.mark.gpu

MAIN_SHAPES = [(2, 256, 3), (3, 384, 5)]
# every regime at the two main shapes; sigma = 0.5 only at one KV tile (no
# rescale) and at five tiles
CASES = [(regime, shape) for regime in REGIMES for shape in MAIN_SHAPES] + [
    ("flat", (1, 128, 1)), ("flat", (1, 640, 2)),
    # upstream gradient of out.sum(): an expanded stride-0 tensor of ones
    ("sum", (2, 256, 3)),
]
TENSORS = ("out", "dq", "dk", "dv")

_CACHE = {}


def _case(regime, shape):
    """GPU inputs, the fp64 reference and the staged reference's metrics,
    computed once per case and shared (never modified) by the tests."""
    key = (regime, shape)
    if key not in _CACHE:
        b, s, nh = shape
        qkv, mask, gy = make_case("flat" if regime == "sum" else regime, b, s, nh)
        if regime == "sum":
            gy = torch.ones_like(gy)
        qkv, gy = qkv.cuda(), gy.cuda()
        mask = None if mask is None else mask.cuda()
        r64 = R.attention_ref64(qkv, mask, gy, nh)
        staged = R.attention_bf16_staged(qkv, mask, gy, nh)
        _CACHE[key] = (qkv, mask, gy, r64, R.attn_metrics(staged, r64, nh))
    return _CACHE[key]


def _run_kernels(qkv, mask, gy, nh, drop_p=0.0, backward_of_sum=False):
    """Forward + backward through the autograd function; returns the result
    and the philox state the forward drew its dropout mask from."""
    from oktopk_amd.ops.fused_attn import _FlashAttention

    x = qkv.clone().requires_grad_(True)
    out = _FlashAttention.apply(x, mask, nh, drop_p, True)
    _, lse, philox, _ = out.grad_fn.saved_tensors
    if backward_of_sum:
        out.sum().backward()
    else:
        out.backward(gy)
    return R.AttnRef(out.detach(), lse, x.grad), philox


def _check(tag, got, r64, staged, nh, names=TENSORS):
    m = R.attn_metrics(got, r64, nh)
    for n in names:
        for i, what in enumerate(("rel_fro", "row_max")):
            print(f"FA_ACC {tag} {n} {what} kernel {m[n][i]:.6g} "
                  f"staged {staged[n][i]:.6g} ratio {m[n][i] / staged[n][i]:.3f}")
    err = (got.lse.double() - r64.lse).abs()
    bound = R.attn_lse_bound(r64.lse)
    print(f"FA_ACC {tag} lse max_err {float(err.max()):.6g} "
          f"max_err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (tag, float((err / bound).max()))
    assert R.attn_over_staged(m, staged, names) == [], (tag, m, staged)


def _id(case):
    regime, (b, s, nh) = case
    return f"{regime}-{b}x{s}x{nh}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_backward(case):
    regime, shape = case
    qkv, mask, gy, r64, staged = _case(regime, shape)
    got, _ = _run_kernels(qkv, mask, gy, shape[2],
                          backward_of_sum=(regime == "sum"))
    _check(_id(case), got, r64, staged, shape[2])


@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_general_mask_case_can_tell_batches_apart(shape):
    """The general-mask case proves something only if reading batch 0's
    mask row for every batch moves the fp64 output by more than the bound."""
    qkv, mask, gy, r64, staged = _case("general", shape)
    wrong = R.attention_ref64(qkv, mask[:1].expand_as(mask), gy, shape[2])
    m = R.attn_metrics(wrong, r64, shape[2])
    bad = R.attn_over_staged(m, staged)
    assert {(n, "rel_fro") for n in TENSORS} <= set(bad), (m, staged)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "sum"], ids=_id)
def test_forward_im2_variant(case, monkeypatch):
    """OKTOPK_FA_IM=2 selects attn_fwd_fa_kernel<2> (128-row query blocks);
    the launcher reads the variable on every call.  Forward only, same
    bounds."""
    from oktopk_amd import _hip_ops

    regime, shape = case
    qkv, mask, gy, r64, staged = _case(regime, shape)
    monkeypatch.setenv("OKTOPK_FA_IM", "2")
    out, lse, _ = _hip_ops.attn_fwd_fa(
        qkv, mask if mask is not None else torch.empty(0, device="cuda"),
        shape[2], 0.0, True, True)
    torch.cuda.synchronize()
    _check("im2-" + _id(case), R.AttnRef(out, lse, r64.dqkv), r64, staged,
           shape[2], names=("out",))


@pytest.mark.parametrize("padded", [False, True], ids=["nomask", "padding"])
@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("drop_p", [0.1, 0.5])
def test_dropout(drop_p, shape, padded):
    """The forward, the dQ kernel and the dK/dV kernel each generate the
    dropout mask themselves.  The mask the forward drew is recovered from
    its saved philox state (dropout_mask_mul_ on ones) and handed to both
    references, which ties all three kernels to one mask at full
    resolution."""
    from oktopk_amd import _hip_ops

    b, s, nh = shape
    qkv, mask, gy, _, _ = _case("padding" if padded else "flat", shape)
    torch.manual_seed(31)
    got, philox = _run_kernels(qkv, mask, gy, nh, drop_p)
    ones = torch.ones(b * nh, s, s, dtype=torch.bfloat16, device="cuda")
    _hip_ops.dropout_mask_mul_(ones, philox, drop_p)
    kept = ones != 0
    # the kernels scale by 1.f / (float)(1 - p)
    inv_keep = float(1.0 / torch.tensor(1.0 - drop_p, dtype=torch.float32))
    keep = kept.float() * inv_keep

    n = kept.numel()
    frac = float(kept.double().mean())
    sigma = (drop_p * (1.0 - drop_p) / n) ** 0.5
    assert abs(frac - (1.0 - drop_p)) <= 5.0 * sigma, (frac, sigma)
    kept4 = kept.view(b, nh, s, s)
    for i in range(b):
        for h in range(1, nh):
            assert not torch.equal(kept4[i, 0], kept4[i, h]), (i, h)
    assert not torch.equal(kept4[0], kept4[1])

    r64 = R.attention_ref64(qkv, mask, gy, nh, keep)
    staged = R.attn_metrics(R.attention_bf16_staged(qkv, mask, gy, nh, keep),
                            r64, nh)
    tag = f"drop{drop_p}-{'padding' if padded else 'flat'}-{b}x{s}x{nh}"
    _check(tag, got, r64, staged, nh)


def test_attn_rowdot():
    """D = rowsum(gO*O) against the fp64 dot product.  A product of two
    bf16 is exact in fp32; a sum of 64 fp32 terms in any order is within
    63 * 2^-24 * sum|term| of the exact sum, hence 64 * 2^-24 * sum_d|gO*O|
    per row."""
    from oktopk_amd import _hip_ops

    b, s, nh = 3, 256, 5
    gen = torch.Generator().manual_seed(41)
    go = torch.randn(b, s, nh * 64, generator=gen).bfloat16().cuda()
    out = torch.randn(b, s, nh * 64, generator=gen).bfloat16().cuda()
    d = _hip_ops.attn_rowdot(go, out, nh)
    assert d.shape == (b * nh, s) and d.dtype == torch.float32
    prod = (go.double() * out.double()).view(b, s, nh, 64)
    ref = prod.sum(-1).permute(0, 2, 1).reshape(b * nh, s)
    bound = 64 * 2.0 ** -24 * prod.abs().sum(-1).permute(0, 2, 1).reshape(b * nh, s)
    err = (d.double() - ref).abs()
    print(f"FA_ACC rowdot max_err/bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), float((err / bound).max())
