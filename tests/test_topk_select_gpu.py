"""HIP topk_select / topk_select_ef (ops/csrc/topk_select.hip) against the
torch reference: idx, val, tau and the residual are bit-equal, t is left
unchanged.  Everything the op computes is an integer count or a copied
value, so there is no tolerance anywhere."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oktopk_amd import ops
from oktopk_amd.ops import reference as R

SIZES = [1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 8191,
         65537, 4_196_358]
DENSITIES = [0.05, 0.001]
TAIL = 70  # the tie class of "tail_ties": inside the last ragged 512-run

KINDS = ["randn", "quant", "tail_ties", "all_equal", "all_zero",
         "bf16", "bf16_quant", "unaligned_residual", "bf16_unaligned"]


def _k(n, density):
    return max(1, int(n * density))


def _bits(x):
    return x.contiguous().view(torch.int32)


def _quant(n, g, scale=4.0):
    return torch.round(torch.randn(n, generator=g) * scale) / scale


_cases = {}


def _case(kind, n):
    """(t, residual, grad) on the CPU, built once per (kind, n)."""
    key = (kind, n)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(n * 31 + len(kind))
    grad = None
    if kind in ("randn", "unaligned_residual"):
        t = torch.randn(n, generator=g)
        res = torch.randn(n, generator=g) * 0.1
    elif kind == "quant":
        # restored lands on multiples of 1/8: tie classes of thousands that
        # straddle lane, wave and block boundaries, `need` ends mid-wave
        t = _quant(n, g)
        res = _quant(n, g) * 0.5
    elif kind == "tail_ties":
        # distinct small magnitudes, one large tie class in the last TAIL
        # elements only
        t = torch.randn(n, generator=g)
        res = torch.zeros(n)
        m = min(n, TAIL)
        sign = torch.where(torch.arange(m) % 3 == 0, -1.0, 1.0)
        t[n - m:] = 16.0 * sign
    elif kind == "all_equal":
        t = torch.full((n,), 0.5)
        res = torch.full((n,), -0.75)
    elif kind == "all_zero":
        t = torch.zeros(n)
        res = torch.zeros(n)
    elif kind in ("bf16", "bf16_unaligned"):
        t = torch.full((n,), 123.0)  # stale: must not be read
        grad = torch.randn(n, generator=g).to(torch.bfloat16)
        res = torch.randn(n, generator=g) * 0.1
    elif kind == "bf16_quant":
        t = torch.full((n,), 123.0)
        grad = _quant(n, g).to(torch.bfloat16)
        res = _quant(n, g) * 0.5
    else:
        raise AssertionError(kind)
    _cases[key] = (t, res, grad)
    return _cases[key]


_refs = {}


def _reference(kind, n, k):
    key = (kind, n, k)
    if key not in _refs:
        t, res, grad = _case(kind, n)
        o_res = res.clone()
        idx, val, tau = R.topk_select_ef(t, o_res, grad, k)
        _refs[key] = (idx, val, tau, o_res)
    return _refs[key]


def _shifted(x):
    """A GPU copy of x whose data pointer is one element off 16-byte
    alignment."""
    buf = torch.empty(x.numel() + 8, dtype=x.dtype, device="cuda")
    view = buf[1:1 + x.numel()]
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    return view


def _ks(kind, n, density):
    ks = [_k(n, density)]
    if kind == "tail_ties":
        ks.append(max(1, min(n, TAIL) // 2))  # tau inside the tail class
    return ks


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_topk_select_ef_matches_reference(kind, n, density):
    t, res, grad = _case(kind, n)
    for k in _ks(kind, n, density):
        o_idx, o_val, o_tau, o_res = _reference(kind, n, k)
        dt = t.cuda()
        dres = _shifted(res) if kind == "unaligned_residual" else res.cuda()
        dgrad = None
        if grad is not None:
            dgrad = _shifted(grad) if kind == "bf16_unaligned" else grad.cuda()
        idx, val, tau = ops.topk_select_ef(dt, dres, dgrad, k)
        assert idx.dtype == torch.int32 and idx.numel() == min(k, n)
        assert torch.equal(idx.cpu(), o_idx)
        assert torch.equal(_bits(val.cpu()), _bits(o_val))
        assert tau == o_tau
        assert torch.equal(_bits(dres.cpu()), _bits(o_res))
        assert torch.equal(_bits(dt.cpu()), _bits(t))


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["randn", "quant", "tail_ties", "all_zero"])
def test_topk_select_plain_matches_reference(kind, n, density):
    t, res, _ = _case(kind, n)
    x = t + res
    for k in _ks(kind, n, density):
        o_idx, o_val, o_tau, _ = _reference(kind, n, k)
        dx = x.cuda()
        idx, val, tau = ops.topk_select(dx, k)
        assert torch.equal(idx.cpu(), o_idx)
        assert torch.equal(_bits(val.cpu()), _bits(o_val))
        assert tau == o_tau
        assert torch.equal(_bits(dx.cpu()), _bits(x))  # writes nothing


@pytest.mark.parametrize("n", [1, 9, 513, 65537])
def test_k_at_and_beyond_n_selects_everything(n):
    t, res, _ = _case("quant", n)
    for k in (n, n + 5):
        o_res = res.clone()
        o_idx, o_val, o_tau = R.topk_select_ef(t, o_res, None, k)
        dres = res.cuda()
        idx, val, tau = ops.topk_select_ef(t.cuda(), dres, None, k)
        assert idx.numel() == n
        assert torch.equal(idx.cpu(), o_idx)
        assert torch.equal(_bits(val.cpu()), _bits(o_val))
        assert tau == o_tau
        assert torch.equal(_bits(dres.cpu()), _bits(o_res))
        assert not dres.any()  # everything sent, nothing kept


def test_argument_checks_on_gpu():
    t = torch.randn(64, device="cuda")
    r = torch.zeros(64, device="cuda")
    with pytest.raises(ValueError):
        ops.topk_select(t, 0)
    with pytest.raises(ValueError):
        ops.topk_select_ef(t, r, None, 0)
    with pytest.raises(TypeError):
        ops.topk_select_ef(t, r.cpu(), None, 3)  # device mismatch
    with pytest.raises(TypeError):
        ops.topk_select_ef(t, r, t.half(), 3)  # grad must be bf16
    with pytest.raises(TypeError):
        ops.topk_select_ef(t, r.double(), None, 3)
    with pytest.raises(TypeError):
        ops.topk_select(t.double(), 3)
