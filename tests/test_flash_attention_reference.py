"""The criteria of test_flash_attention_accuracy_gpu.py, shown without a GPU
to be able to fail.

The GPU file bounds each metric of the kernels' result by
R.ATTN_STAGED_FACTOR times the same metric of R.attention_bf16_staged.  Here
the two references are checked against each other, and a set of mutants of
the staged reference — each a way the hand-written kernels could be subtly
wrong — must each break that bound on the tensors it touches."""
import pytest
import torch

from attn_cases import make_case, random_keep
from oktopk_amd.ops import reference as R

NH = 3


@pytest.fixture(scope="module")
def plain():
    """General per-batch mask, no dropout, at (2, 256, 3)."""
    qkv, mask, gy = make_case("general", 2, 256, NH)
    return qkv, mask, gy, None


@pytest.fixture(scope="module")
def peaked():
    """sigma = 2.0, no mask: the regime in which D = rowsum(gO*O) is of the
    size of dP.  Under flat attention D is an average of many dP of either
    sign and so small that a 5 % error in it stays inside the bound."""
    qkv, mask, gy = make_case("peaked", 2, 256, NH)
    return qkv, mask, gy, None


@pytest.fixture(scope="module")
def dropped():
    """The same inputs under a dropout mask of p = 0.1."""
    qkv, mask, gy = make_case("general", 2, 256, NH)
    keep = random_keep(2, NH, 256, 0.1, torch.Generator().manual_seed(7))
    return qkv, mask, gy, keep


_REF_CACHE = {}


def _refs(case):
    """(ref64, metrics of the unmutated staged reference), once per case."""
    key = id(case)
    if key not in _REF_CACHE:
        qkv, mask, gy, keep = case
        r64 = R.attention_ref64(qkv, mask, gy, NH, keep)
        clean = R.attn_metrics(_staged(case), r64, NH)
        _REF_CACHE[key] = (r64, clean)
    return _REF_CACHE[key]


def _staged(case, mut=None):
    """R.attention_bf16_staged, step by step, with one deliberate error."""
    qkv, mask, gy, keep = case
    q, k, v, go, m, kp, scale = R.attn_staged_inputs(qkv, mask, gy, NH, keep)
    if mut == "mask_batch0":        # every batch reads batch 0's mask row
        m = m[:1].expand_as(m)
    o, lse, o32 = R.attn_staged_forward(q, k, v, m, kp, scale)
    dvec = (go * o).sum(dim=-1)
    if mut == "d_fp32_o_x1.05":     # D from the unrounded O, 5 % off
        dvec = (go * o32).sum(dim=-1) * 1.05
    # the dQ kernel and the dK/dV kernel each recompute P and dS themselves
    m_kv = None if mut == "dkv_no_mask" else m
    ds_scale = scale * 1.02 if mut == "ds_scale_x1.02" else scale
    p_q = R.attn_staged_p(q, k, lse, m, scale)
    p_kv = R.attn_staged_p(q, k, lse, m_kv, scale)
    ds_q = R.attn_staged_ds(p_q, go, v, dvec, kp, ds_scale)
    ds_kv = R.attn_staged_ds(p_kv, go, v, dvec, kp,
                             1.0 if mut == "dk_no_scale" else ds_scale)
    if mut == "dq_skip_last_tile":  # the last 128-key tile never accumulated
        dq = R.attn_staged_dq(ds_q[..., :-128], k[..., :-128, :])
    else:
        dq = R.attn_staged_dq(ds_q, k)
    if mut == "dq_zero":
        dq = torch.zeros_like(dq)
    if mut == "dq_row_dup":         # one row written from its neighbour
        dq = dq.clone()
        dq[1, 2, 37] = dq[1, 2, 36]
    dk = R.attn_staged_dk(ds_kv, q)
    kp_v = kp.transpose(-1, -2) if mut == "dv_keep_transposed" else kp
    dv = R.attn_staged_dv(p_kv, go, kp_v)
    if mut == "lse_plus_2^-8":
        lse = lse + 2.0 ** -8
    return R.attn_staged_result(o, lse, dq, dk, dv)


def _lse_ok(res, r64):
    err = (res.lse.double() - r64.lse).abs()
    return bool((err <= R.attn_lse_bound(r64.lse)).all())


@pytest.mark.parametrize("shape,regime", [
    ((1, 128, 1), "flat"), ((2, 256, 3), "flat"), ((3, 384, 5), "flat"),
    ((2, 256, 3), "general"), ((3, 384, 5), "general"),
    ((2, 256, 3), "padding"), ((3, 384, 5), "padding")])
def test_references_agree(shape, regime):
    """Sanity cap on the references themselves (not on the kernel): at
    sigma = 0.5 the staged reference sits within rel_fro 0.01 of fp64 on
    every tensor, and its LSE (no bf16 anywhere) within the LSE bound."""
    b, s, nh = shape
    qkv, mask, gy = make_case(regime, b, s, nh)
    r64 = R.attention_ref64(qkv, mask, gy, nh)
    st = R.attention_bf16_staged(qkv, mask, gy, nh)
    for name, (fro, _) in R.attn_metrics(st, r64, nh).items():
        assert fro < 0.01, (name, fro)
    assert _lse_ok(st, r64)
    # the step-by-step composition the mutants use is the same function
    if shape == (2, 256, 3) and regime == "general":
        again = _staged((qkv, mask, gy, None))
        assert torch.equal(again.dqkv, st.dqkv) and torch.equal(again.out, st.out)


def test_references_agree_under_dropout(dropped):
    qkv, mask, gy, keep = dropped
    r64, clean = _refs(dropped)
    st = R.attention_bf16_staged(qkv, mask, gy, NH, keep)
    for name, (fro, _) in R.attn_metrics(st, r64, NH).items():
        assert fro < 0.01, (name, fro)
    assert R.attn_over_staged(clean, clean) == []


# mutant -> (tensor, metric) pairs that must exceed the bound; metric None
# means either of the two
MUTANTS = {
    "ds_scale_x1.02": [("dq", None), ("dk", None)],
    "dk_no_scale": [("dk", None)],
    "dq_zero": [("dq", None)],
    "dq_row_dup": [("dq", "row_max")],
    "dq_skip_last_tile": [("dq", None)],
    "mask_batch0": [("out", None), ("dq", None), ("dk", None), ("dv", None)],
    "dkv_no_mask": [("dk", None), ("dv", None)],
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_breaks_bound(plain, mut):
    r64, clean = _refs(plain)
    got = R.attn_metrics(_staged(plain, mut), r64, NH)
    bad = R.attn_over_staged(got, clean)
    for name, what in MUTANTS[mut]:
        hits = [w for n, w in bad if n == name]
        assert hits and (what is None or what in hits), (mut, name, got, clean)
    # and it breaks nothing it does not touch
    touched = {n for n, _ in MUTANTS[mut]}
    if mut in ("ds_scale_x1.02", "dk_no_scale", "dq_zero", "dq_row_dup",
               "dq_skip_last_tile"):
        assert {n for n, _ in bad} <= touched, (mut, bad)


def test_mutant_d_from_fp32_o(peaked):
    r64, clean = _refs(peaked)
    got = R.attn_metrics(_staged(peaked, "d_fp32_o_x1.05"), r64, NH)
    assert {n for n, _ in R.attn_over_staged(got, clean)} == {"dq", "dk"}, (
        got, clean)


def test_mutant_keep_transposed_in_dv(dropped):
    """The three kernels each generate the dropout mask themselves: a dV
    path that indexed it (key, query) for (query, key) is caught."""
    r64, clean = _refs(dropped)
    got = R.attn_metrics(_staged(dropped, "dv_keep_transposed"), r64, NH)
    assert {n for n, _ in R.attn_over_staged(got, clean)} == {"dv"}, (got, clean)


def test_mutant_lse_offset(plain):
    r64, _ = _refs(plain)
    assert _lse_ok(_staged(plain), r64)
    assert not _lse_ok(_staged(plain, "lse_plus_2^-8"), r64)


def test_lse_bound_values():
    b = R.attn_lse_bound(torch.tensor([0.0, -3.0, 100.0, -10000.0],
                                      dtype=torch.float64))
    assert b.tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9]


def test_row_max_with_mostly_zero_reference_rows():
    """More than half of the reference rows exactly zero (masked keys' dK
    and dV): the median falls back to the nonzero rows."""
    ref = torch.zeros(10, 64, dtype=torch.float64)
    ref[:4] = 1.0
    x = ref.clone()
    x[7, 0] = 4.0
    assert R.attn_row_max(x, ref) == pytest.approx(4.0 / 8.0)
    assert R.attn_rel_fro(x, ref) == pytest.approx(4.0 / 16.0)


def test_old_packed_allclose_accepts_zero_dq_dk():
    """Why this file exists: the criterion of test_flash_attention_autograd,
    allclose(atol=0.1, rtol=0.05) on the packed gradient, at that test's
    shape, seed and scaling (s = 256), accepts dQ = dK = 0 — every
    reference dQ and dK element is below atol.  The per-tensor metrics
    reject it."""
    torch.manual_seed(14)
    b, s, nh = 2, 256, 4
    qkv = (torch.randn(b, s, 3 * nh * 64) * 0.5).bfloat16()
    gy = torch.randn(b, s, nh * 64).bfloat16()
    r64 = R.attention_ref64(qkv, None, gy, nh)
    ref = r64.dqkv.float()
    wrong = ref.clone().view(b, s, 3, nh, 64)
    wrong[:, :, :2] = 0.0
    wrong = wrong.view(b, s, -1)
    assert ref.view(b, s, 3, nh, 64)[:, :, :2].abs().max() < 0.1
    assert torch.allclose(wrong, ref, atol=0.1, rtol=0.05)
    st = R.attention_bf16_staged(qkv, None, gy, nh)
    bad = R.attn_over_staged(
        R.attn_metrics(R.AttnRef(r64.out, r64.lse, wrong), r64, nh),
        R.attn_metrics(st, r64, nh))
    assert {n for n, _ in bad} == {"dq", "dk"}
