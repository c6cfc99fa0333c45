"""Ok-Topk round-2 tail (ops.round2_tail_ / ops.round2_tail_wire_) on the
CPU: the torch references against a brute-force composition, the wire form
against the pair form, the engine with OkTopkConfig.device_round2 against the
host composition over gloo, and the sparse hand-over on exact iterations.
Every comparison is bit for bit."""
import os

import pytest
import torch

from conftest import run_dist
from oktopk_amd import ops
from oktopk_amd.config import EngineConfig, OkTopkConfig
from oktopk_amd.ops import reference as ref


def bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def sorted_unique(n, m, gen):
    return torch.randperm(n, generator=gen)[:m].sort().values.to(torch.int32)


def brute(residual, idx, all_idx, all_val, k):
    """The op by other means: stable torch.sort of the magnitude bits for the
    selection, a Python set intersection for the credit.  Returns (g_idx,
    g_val, tau, residual_after)."""
    S = all_idx.numel()
    if k is None or S == 0:
        pos, tau = torch.arange(S), None
    else:
        mag = (bits(all_val) & 0x7FFFFFFF).long()
        # stable + descending: equal magnitudes stay in position order, so
        # the first min(k, S) are topk_select's choice
        order = torch.sort(mag, descending=True, stable=True).indices
        kk = min(k, S)
        pos = order[:kk].sort().values
        tau = float((mag[order[kk - 1]]).to(torch.int32).reshape(1)
                    .view(torch.float32).item())
    g_idx, g_val = all_idx[pos], all_val[pos]
    after = residual.clone()
    n = residual.numel()
    for j in sorted(set(g_idx.tolist()) & set(idx.tolist())):
        if 0 <= j < n:
            after[j] = 0.0
    return g_idx, g_val, tau, after


def check_case(fn, residual, idx, all_idx, all_val, k):
    """fn(residual, idx, all_idx, all_val, k) against brute(), in bits,
    including the whole residual; plus the dense-scatter view of the
    selection."""
    want_idx, want_val, want_tau, want_res = brute(residual, idx, all_idx,
                                                   all_val, k)
    res = residual.clone()
    g_idx, g_val, tau = fn(res, idx, all_idx, all_val, k)
    assert g_idx.dtype == torch.int32 and g_val.dtype == torch.float32
    assert torch.equal(g_idx.cpu(), want_idx)
    assert same_bits(g_val.cpu(), want_val)
    assert tau == want_tau and (tau is None or isinstance(tau, float))
    assert same_bits(res.cpu(), want_res)
    if g_idx.numel() > 1:
        assert bool((g_idx[1:] > g_idx[:-1]).all())
    n = residual.numel()
    inb = (want_idx >= 0) & (want_idx < n)
    dense_want = torch.zeros(n).index_put_((want_idx[inb].long(),), want_val[inb])
    gi, gv = g_idx.cpu(), g_val.cpu()
    dense_got = torch.zeros(n).index_put_((gi[inb].long(),), gv[inb])
    assert same_bits(dense_got, dense_want)
    return g_idx, g_val, tau


def make_case(n, S, m, seed, overlap="random", values="randn"):
    gen = torch.Generator().manual_seed(seed)
    all_idx = sorted_unique(n, S, gen)
    if overlap == "identical":
        idx = all_idx.clone()
    elif overlap == "disjoint":
        rest = torch.ones(n, dtype=torch.bool)
        rest[all_idx.long()] = False
        pool = rest.nonzero().reshape(-1)
        idx = pool[torch.randperm(pool.numel(), generator=gen)[:m]] \
            .sort().values.to(torch.int32)
    else:
        idx = sorted_unique(n, m, gen)
    if values == "randn":
        all_val = torch.randn(S, generator=gen)
    elif values == "one_magnitude":  # the tie rule decides everything
        sign = torch.randint(0, 2, (S,), generator=gen) * 2 - 1
        all_val = 0.75 * sign.float()
    elif values == "few":  # a handful of magnitudes, as bf16 wire values tie
        lv = torch.tensor([0.0, -0.0, 0.5, -0.5, 1.0, 2.0, -2.0])
        all_val = lv[torch.randint(0, lv.numel(), (S,), generator=gen)]
    else:
        raise AssertionError(values)
    residual = torch.randn(n, generator=gen) + 3.0  # no zeros to start with
    return residual, idx, all_idx, all_val


K_OF = {"none": lambda S: None, "1": lambda S: 1, "S-1": lambda S: S - 1,
        "S": lambda S: S, "S+5": lambda S: S + 5, "S//3": lambda S: S // 3}


@pytest.mark.parametrize("kname", list(K_OF))
@pytest.mark.parametrize("overlap", ["random", "identical", "disjoint"])
@pytest.mark.parametrize("values", ["randn", "one_magnitude", "few"])
def test_reference_matches_brute_force(kname, overlap, values):
    residual, idx, all_idx, all_val = make_case(1000, 300, 280, 11, overlap, values)
    k = K_OF[kname](300)
    check_case(ops.round2_tail_, residual, idx, all_idx, all_val, k)
    check_case(ref.round2_tail_, residual, idx, all_idx, all_val, k)


def test_reference_tie_class_filled_from_lowest_position():
    residual, idx, all_idx, all_val = make_case(500, 64, 64, 5, "identical",
                                                "one_magnitude")
    g_idx, g_val, tau = check_case(ops.round2_tail_, residual, idx, all_idx,
                                   all_val, 10)
    assert torch.equal(g_idx, all_idx[:10]) and tau == 0.75


def test_reference_signed_zeros():
    all_idx = torch.tensor([1, 4, 6, 9, 12], dtype=torch.int32)
    all_val = torch.tensor([0.0, -0.0, 0.0, -0.0, 1.0])
    idx = torch.tensor([4, 6, 12, 13], dtype=torch.int32)
    residual = torch.full((16,), -1.5)
    g_idx, g_val, tau = check_case(ops.round2_tail_, residual, idx, all_idx,
                                   all_val, 3)
    # +0.0 and -0.0 share the key 0: the two lowest positions fill the class
    assert g_idx.tolist() == [1, 4, 12] and tau == 0.0
    assert torch.equal(torch.signbit(g_val), torch.tensor([False, True, False]))
    res = residual.clone()
    ops.round2_tail_(res, idx, all_idx, all_val, 3)
    assert not bool(torch.signbit(res[[4, 12]]).any())  # the credit is +0.0


@pytest.mark.parametrize("k", [None, 1, 7])
def test_reference_empty_inputs(k):
    residual, idx, all_idx, all_val = make_case(200, 50, 40, 3)
    e_i, e_v = all_idx[:0], all_val[:0]
    # S == 0: the (empty) lists come back as they are, tau is None
    g_idx, g_val, tau = check_case(ops.round2_tail_, residual, idx, e_i, e_v, k)
    assert g_idx is e_i and g_val is e_v and tau is None
    # empty local selection: selection as usual, nothing credited
    check_case(ops.round2_tail_, residual, idx[:0], all_idx, all_val, k)


def test_threshold_mode_returns_inputs_uncopied():
    residual, idx, all_idx, all_val = make_case(200, 50, 40, 4)
    g_idx, g_val, tau = ops.round2_tail_(residual, idx, all_idx, all_val)
    assert g_idx is all_idx and g_val is all_val and tau is None


def test_out_of_range_matches_are_dropped():
    all_idx = torch.tensor([2, 7, 40, 90], dtype=torch.int32)
    all_val = torch.tensor([1.0, 2.0, 3.0, 4.0])
    idx = torch.tensor([7, 40, 90], dtype=torch.int32)
    residual = torch.ones(40)  # 40 and 90 lie outside
    for k in (None, 4, 2):
        check_case(ops.round2_tail_, residual, idx, all_idx, all_val, k)
    res = residual.clone()
    ops.round2_tail_(res, idx, all_idx, all_val)
    assert res[7] == 0.0 and int((res == 0).sum()) == 1


def test_argument_errors():
    residual, idx, all_idx, all_val = make_case(100, 20, 10, 2)
    buf, counts = ref.pack_regions(all_idx, all_val,
                                   torch.tensor([0, 100]), False)
    for bad in (
        lambda: ops.round2_tail_(residual, idx, all_idx, all_val, 0),
        lambda: ops.round2_tail_(residual, idx, all_idx, all_val, -3),
        lambda: ops.round2_tail_(residual.double(), idx, all_idx, all_val),
        lambda: ops.round2_tail_(residual, idx.long(), all_idx, all_val),
        lambda: ops.round2_tail_(residual, idx, all_idx.long(), all_val),
        lambda: ops.round2_tail_(residual, idx, all_idx, all_val.double()),
        lambda: ops.round2_tail_(residual, idx, all_idx, all_val[:-1], 3),
        lambda: ops.round2_tail_wire_(residual, idx, buf, counts, False, 0),
        lambda: ops.round2_tail_wire_(residual, idx, buf.float(), counts, False),
        lambda: ops.round2_tail_wire_(residual, idx, buf, [counts[0] + 1], False),
    ):
        with pytest.raises(ValueError):
            bad()


# -- wire form against pair form ------------------------------------------

def wire_case(n, seg_counts, m, seed, wire_bf16, values="randn"):
    """Rank-ordered segments over disjoint ascending index ranges, packed in
    the wire layout by the codec reference."""
    S = sum(seg_counts)
    residual, idx, all_idx, all_val = make_case(n, S, m, seed, values=values)
    if not seg_counts:  # nobody gathered anything
        return residual, idx, torch.zeros(0, dtype=torch.int32), []
    cuts = [0]
    for c in seg_counts:
        cuts.append(cuts[-1] + c)
    bounds = [0] + [int(all_idx[c]) if c < S else n for c in cuts[1:-1]] + [n]
    buf, counts = ref.pack_regions(all_idx, all_val,
                                   torch.tensor(bounds, dtype=torch.int64),
                                   wire_bf16)
    assert counts == list(seg_counts)
    return residual, idx, buf, counts


WIRE_SEGS = [[37], [0, 5, 0, 12, 1], [3, 0, 0, 7, 9, 1, 0, 11], [0, 0], []]


@pytest.mark.parametrize("wire_bf16", [False, True])
@pytest.mark.parametrize("segs", WIRE_SEGS)
@pytest.mark.parametrize("kname", ["none", "1", "S-1", "S", "S+5", "S//3"])
def test_wire_form_equals_pair_form(wire_bf16, segs, kname):
    S = sum(segs)
    k = K_OF[kname](S)
    if k is not None and k < 1:
        k = 1
    # bf16: few distinct magnitudes, so the k-th magnitude ties on purpose
    residual, idx, buf, counts = wire_case(
        400, segs, 30, 17, wire_bf16, "few" if wire_bf16 else "randn")
    if wire_bf16:
        assert any(c % 2 for c in counts) or S == 0  # pad half-words present
    all_idx, all_val = ops.unpack_segments(buf, counts, wire_bf16)
    r_pair, r_wire = residual.clone(), residual.clone()
    p_idx, p_val, p_tau = ops.round2_tail_(r_pair, idx, all_idx, all_val, k)
    w_idx, w_val, w_tau = ops.round2_tail_wire_(r_wire, idx, buf, counts,
                                                wire_bf16, k)
    assert torch.equal(w_idx, p_idx) and same_bits(w_val, p_val)
    assert w_tau == p_tau and same_bits(r_wire, r_pair)
    if k is None:
        assert torch.equal(w_idx, all_idx) and same_bits(w_val, all_val)
    check_case(lambda r, i, a, v, kk: ops.round2_tail_wire_(
        r, i, buf, counts, wire_bf16, kk), residual, idx, all_idx, all_val, k)


# -- config / CLI ------------------------------------------------------------

def test_flag_defaults_off_and_reaches_config():
    from oktopk_amd.train import build_argparser

    assert OkTopkConfig().device_round2 is False
    assert EngineConfig.preset("bert", device_round2=True).oktopk.device_round2
    assert build_argparser().parse_args([]).device_round2 is False
    assert build_argparser().parse_args(["--device-round2"]).device_round2 is True


# -- engine: flag on against flag off -----------------------------------------

N = 8192
DENSITY = 0.02
ITERS = 8
VARIANTS = {
    "plain": {},
    "chunked": {"pipeline_chunks": 2},
    "balanced": {"balanced_allgather": True},
    "device_wire": {"device_wire": True},
}


def engine_grad(rank, it):
    g = torch.Generator().manual_seed(7000 * rank + 13 * it + 5)
    return torch.randn(N, generator=g)


def engine_equivalence(rank, device, configs):
    """Worker: for every (label, OkTopkConfig kwargs) in `configs`, run the
    engine with device_round2 on and off over the same gradients and compare
    outputs, residuals and thresholds in bits after every iteration."""
    import torch.distributed as dist

    from oktopk_amd import AllReducer, Comm, ops as eops

    if device == "cuda":
        torch.cuda.set_device(0)
    seen = []  # (S, k) of every exact call the flagged engine makes

    def guard(all_val, k):
        # torch.topk leaves ties unspecified, so the comparison is only
        # defined where the k-th and (k+1)-th magnitudes differ
        if k is None:
            return
        S = all_val.numel()
        seen.append((S, k))
        if S > k:
            mag = torch.sort(all_val.abs(), descending=True).values
            assert mag[k - 1] != mag[k], "k-th / (k+1)-th tie: pick another seed"

    pair_op, wire_op = eops.round2_tail_, eops.round2_tail_wire_

    def pair_guarded(residual, idx, all_idx, all_val, k=None):
        guard(all_val, k)
        return pair_op(residual, idx, all_idx, all_val, k)

    def wire_guarded(residual, idx, buf, counts, wire_bf16, k=None):
        guard(eops.unpack_segments(buf, counts, wire_bf16)[1], k)
        return wire_op(residual, idx, buf, counts, wire_bf16, k)

    eops.round2_tail_, eops.round2_tail_wire_ = pair_guarded, wire_guarded
    try:
        for label, kw in configs:
            def build(flag):
                return AllReducer(Comm(dist.group.WORLD), EngineConfig(
                    compressor="oktopk", density=DENSITY, wire_dtype="fp32",
                    oktopk=OkTopkConfig(
                        dense_warmup_iters=0,
                        local_threshold_recompute_interval=4,
                        global_threshold_recompute_interval=3,
                        region_repartition_interval=2,
                        device_round2=flag, **kw)))

            off, on = build(False), build(True)
            del seen[:]
            for it in range(ITERS):
                t = engine_grad(rank, it).to(device)
                a = off.run("w", t.clone())
                b = on.run("w", t.clone())
                assert same_bits(a, b), (label, it)
                assert sorted(off.states) == sorted(on.states)
                for name, st in on.states.items():
                    ref_st = off.states[name]
                    assert same_bits(st.residual, ref_st.residual), (label, it, name)
                    assert st.tau_global == ref_st.tau_global, (label, it, name)
                    assert st.mask is None, (label, it, name)
            assert any(st.tau_global > 0.0 for st in on.states.values())
            # the exact iterations really truncate
            assert seen and all(S > k for S, k in seen), (label, seen)
    finally:
        eops.round2_tail_, eops.round2_tail_wire_ = pair_op, wire_op


@pytest.mark.parametrize("world", [2, 3, 4])
def test_engine_device_round2_equals_host_composition(world):
    run_dist(engine_equivalence, world,
             args=("cpu", list(VARIANTS.items())))


# -- the sparse hand-over covers the exact iterations --------------------------

_TINY = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=2,
             intermediate_size=128)
_STEPS = 5


def _train(comm, sparse_step):
    """5 steps of a tiny BERT with device_round2 on; iterations 0 and 3 are
    exact ones.  Returns what each step handed over and the optimizer state
    after every step."""
    from oktopk_amd.trainer import Trainer

    os.environ["OKTOPK_SPARSE_STEP"] = sparse_step
    try:
        torch.manual_seed(0)
        cfg = EngineConfig.preset(
            "bert", compressor="oktopk", density=0.01, dense_warmup_iters=0,
            local_threshold_recompute_interval=4,
            global_threshold_recompute_interval=3, device_round2=True)
        tr = Trainer("bert_base", batch_size=2, seq_len=16, comm=comm, cfg=cfg,
                     dtype="fp32", model_kwargs=_TINY)
        took, snaps = [], []
        for _ in range(_STEPS):
            tr.step()
            opt = tr.opt
            took.append(opt.reducer.sparse_result)
            snaps.append((opt.flat_param.clone(), opt.exp_avg.clone(),
                          opt.exp_avg_sq.clone(),
                          opt.reducer.states["flat"].residual.clone()))
    finally:
        os.environ.pop("OKTOPK_SPARSE_STEP", None)
    assert tr.opt.reducer.states["flat"].mask is None
    return took, snaps


def _assert_handover(comm):
    P = 1 if comm is None else comm.size
    took_on, on = _train(comm, "1")
    took_off, off = _train(comm, "0")
    # every step hands over sparse, the exact iterations (0, 3) included
    assert all(sg is not None for sg in took_on)
    assert all(sg is None for sg in took_off)
    for it in (0, 3):
        sg = took_on[it]
        assert sg.scale == 1.0 / P and sg.tau == -1.0
        assert sg.idx.dtype == torch.int32
        assert bool((sg.idx[1:] > sg.idx[:-1]).all())
    for step, (a, b) in enumerate(zip(on, off)):
        for x, y, name in zip(a, b, ("param", "exp_avg", "exp_avg_sq",
                                     "residual")):
            assert torch.equal(x, y), (step, name)
    assert float(on[-1][1].abs().max()) > 0.0  # the steps did move something


def test_handover_on_exact_iterations_world1():
    _assert_handover(None)


def _handover_world2(rank):
    import torch.distributed as dist

    from oktopk_amd.comm import Comm

    _assert_handover(Comm(dist.group.WORLD))


def test_handover_on_exact_iterations_world2():
    run_dist(_handover_world2, 2)
