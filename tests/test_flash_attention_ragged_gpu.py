"""Flash attention at seq % 128 != 0 (the ragged instantiations of
attention_fa.hip, opt-in OKTOPK_FA_ANY_SEQ=1) against the fp64 reference,
per tensor, with the criterion of test_flash_attention_accuracy_gpu.py:
out, dQ, dK, dV within R.ATTN_STAGED_FACTOR of R.attention_bf16_staged on
rel_fro and row_max, lse within R.attn_lse_bound.

The kernels' inputs are the leading b batches of (b+1)-batch buffers whose
last batch is NaN, so a read past a batch's last row or past the tensor
shows up as a NaN in the result."""
import math

import pytest
import torch

from attn_cases import MASKED, make_case
from oktopk_amd.ops import reference as R

pytestmark = pytest.mark.gpu

# (b, s, nh): s < 16 and s % 4 != 0; one partial query block with a partial
# 16-key fragment; a full tile + 2 keys; a 72-key tail whose last query
# block has 8 rows; two full tiles + 1 key
SHAPES = [(2, 5, 2), (2, 50, 3), (2, 130, 2), (3, 200, 3), (1, 257, 2)]
REGIMES = ("flat", "general", "peaked", "tailpad")
TENSORS = ("out", "dq", "dk", "dv")


@pytest.fixture(autouse=True)
def _any_seq(monkeypatch):
    monkeypatch.setenv("OKTOPK_FA_ANY_SEQ", "1")


def _nan_tailed(t):
    """t on the GPU as the leading batches of a buffer with one NaN batch
    more."""
    buf = torch.full((t.shape[0] + 1,) + t.shape[1:], float("nan"),
                     dtype=t.dtype, device="cuda")
    buf[:-1] = t
    return buf[:-1]


def _inputs(regime, shape):
    b, s, nh = shape
    qkv, mask, gy = make_case("flat" if regime == "tailpad" else regime, b, s, nh)
    if regime == "tailpad":  # batch i masks its last 1 + i keys
        mask = torch.zeros(b, s)
        for i in range(b):
            mask[i, s - (1 + i):] = MASKED
        mask = mask.bfloat16()
    return (_nan_tailed(qkv), None if mask is None else _nan_tailed(mask),
            _nan_tailed(gy))


def _run_kernels(qkv, mask, gy, nh, drop_p=0.0):
    from oktopk_amd.ops.fused_attn import _FlashAttention

    x = qkv.detach().requires_grad_(True)  # no clone: keeps the NaN batch behind
    out = _FlashAttention.apply(x, mask, nh, drop_p, True)
    _, lse, philox, _ = out.grad_fn.saved_tensors
    out.backward(gy)
    return R.AttnRef(out.detach(), lse, x.grad), philox


def _check(tag, got, qkv, mask, gy, nh, keep=None):
    r64 = R.attention_ref64(qkv, mask, gy, nh, keep)
    staged = R.attn_metrics(R.attention_bf16_staged(qkv, mask, gy, nh, keep), r64, nh)
    for t in got:
        assert bool(torch.isfinite(t).all()), tag
    m = R.attn_metrics(got, r64, nh)
    for n in TENSORS:
        for i, what in enumerate(("rel_fro", "row_max")):
            print(f"FA_RAGGED {tag} {n} {what} kernel {m[n][i]:.6g} "
                  f"staged {staged[n][i]:.6g} ratio {m[n][i] / staged[n][i]:.3f}")
    err = (got.lse.double() - r64.lse).abs()
    bound = R.attn_lse_bound(r64.lse)
    print(f"FA_RAGGED {tag} lse max_err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (tag, float((err / bound).max()))
    assert R.attn_over_staged(m, staged, TENSORS) == [], (tag, m, staged)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("regime", REGIMES)
def test_forward_backward(regime, shape):
    qkv, mask, gy = _inputs(regime, shape)
    got, _ = _run_kernels(qkv, mask, gy, shape[2])
    _check(f"{regime}-{shape}", got, qkv, mask, gy, shape[2])


def test_single_key():
    """s = 1: softmax over one key is 1, so out is V and dV is gy, bit for
    bit, and lse is the one score."""
    b, s, nh = 2, 1, 2
    qkv, _, gy = _inputs("flat", (b, s, nh))
    got, _ = _run_kernels(qkv, None, gy, nh)
    q, k, v = (t.reshape(b, s, nh * 64) for t in R.attn_split_heads(qkv, nh))
    g = got.dqkv.view(b, s, 3, nh * 64)
    assert torch.equal(got.out, v)
    assert torch.equal(g[:, :, 2], gy)
    assert bool(torch.isfinite(g).all())
    score = (q.double() * k.double()).view(b, nh, 64).sum(-1) / math.sqrt(64)
    err = (got.lse.double() - score.reshape(b * nh, s)).abs()
    assert bool((err <= R.attn_lse_bound(score.reshape(b * nh, s))).all())


@pytest.mark.parametrize("shape", [(2, 50, 3), (2, 200, 2)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("drop_p", [0.1, 0.5])
def test_dropout(drop_p, shape):
    """As test_dropout of the dense suite: the mask the forward drew is
    recovered with dropout_mask_mul_ and handed to the references, which
    ties the forward, dQ, the key-parallel cooperative mask and the
    regeneration kernel to one counter mapping at s % 4 != 0."""
    from oktopk_amd import _hip_ops

    b, s, nh = shape
    qkv, mask, gy = _inputs("flat", shape)
    torch.manual_seed(31)
    got, philox = _run_kernels(qkv, mask, gy, nh, drop_p)
    ones = torch.ones(b * nh, s, s, dtype=torch.bfloat16, device="cuda")
    _hip_ops.dropout_mask_mul_(ones, philox, drop_p)
    kept = ones != 0
    # the kernels scale by 1.f / (float)(1 - p)
    inv_keep = float(1.0 / torch.tensor(1.0 - drop_p, dtype=torch.float32))

    frac = float(kept.double().mean())
    sigma = (drop_p * (1.0 - drop_p) / kept.numel()) ** 0.5
    assert abs(frac - (1.0 - drop_p)) <= 5.0 * sigma, (frac, sigma)
    kept4 = kept.view(b, nh, s, s)
    for i in range(b):
        for h in range(1, nh):
            assert not torch.equal(kept4[i, 0], kept4[i, h]), (i, h)
    assert not torch.equal(kept4[0], kept4[1])
    _check(f"drop{drop_p}-{shape}", got, qkv, mask, gy, nh, kept.float() * inv_keep)


def test_dense_shape_bits_unchanged(monkeypatch):
    """seq % 128 == 0 launches the dense kernels whatever the switch says."""
    qkv, _, gy = make_case("flat", 2, 256, 3)
    qkv, gy = qkv.cuda(), gy.cuda()
    res = []
    for switch in ("1", None):
        if switch is None:
            monkeypatch.delenv("OKTOPK_FA_ANY_SEQ")
        torch.manual_seed(7)
        res.append(_run_kernels(qkv, None, gy, 3, 0.1)[0])
    for x, y in zip(*res):
        assert torch.equal(x, y)


def test_gate(monkeypatch):
    from oktopk_amd.ops.fused_attn import fused_attn_available as avail

    x = torch.empty(1, 1, 3 * 2 * 64, dtype=torch.bfloat16, device="cuda")
    assert avail(x, 2, 200, 0.1) and avail(x, 2, 256, 0.1)
    monkeypatch.setenv("OKTOPK_FUSED_ATTN", "0")
    assert not avail(x, 2, 200, 0.1) and not avail(x, 2, 256, 0.1)
    monkeypatch.delenv("OKTOPK_FUSED_ATTN")
    monkeypatch.delenv("OKTOPK_FA_ANY_SEQ")
    assert not avail(x, 2, 200, 0.1) and avail(x, 2, 256, 0.1)
