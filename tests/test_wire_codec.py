"""Sparse wire codec, torch reference implementations (CPU).

ops.reference.pack_regions / unpack_segments / unpack_scatter_add_ against
the engine's host construction (searchsorted cuts, AllReducer._pack per
slice, cat; AllReducer._unpack, subtract, scatter_add_), and the
OkTopkConfig.device_wire engine path against the host path over gloo.
"""
import pytest
import torch

from conftest import run_dist
from oktopk_amd import AllReducer, Comm, EngineConfig
from oktopk_amd import ops
from oktopk_amd.ops import reference as R

SHAPES = [(1, 7), (2, 0), (3, 11), (8, 5), (8, 257), (64, 300)]
WIRES = [False, True]

# fp32 bit patterns the bf16 conversion must get right: +-0, +-inf, a
# denormal, two exact round-to-even ties (down and up), the largest finite
# value (rounds to inf)
SPECIAL_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001,
                0x3F808000, 0x3F818000, 0x7F7FFFFF]


def special_values():
    return torch.tensor(SPECIAL_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)


def selection(m, n, seed):
    """m ascending unique int32 indices below n with fp32 values (the
    special bit patterns first, then normals)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(n, generator=g)[:m].sort().values.to(torch.int32)
    val = torch.randn(m, generator=g)
    sp = special_values()[:m]
    val[: sp.numel()] = sp
    return idx, val


def boundary_tables(P, idx, n):
    """Named [P+1] int64 boundary tables: the uniform split plus every
    edge the splitting rule has."""
    out = {}
    b = torch.tensor([i * (n // P) for i in range(P)] + [n], dtype=torch.int64)
    out["uniform"] = b
    if P >= 2 and idx.numel():
        e = b.clone()  # a boundary equal to an index -> upper region
        e[1:P] = int(idx[idx.numel() // 2])
        out["on_index"] = e
        z = b.clone()  # interior boundary at 0: region 0 is empty
        z[1] = 0
        out["at_zero"] = z
        t = b.clone()  # interior boundary at n: the last region is empty
        t[P - 1] = n
        out["at_n"] = t
    if P >= 3:
        q = b.clone()  # two equal boundaries: an empty region in the middle
        q[2] = q[1]
        out["equal"] = q
    return out


def engine(wire_bf16):
    return AllReducer(Comm(None), EngineConfig(
        wire_dtype="bf16" if wire_bf16 else "fp32"))


def host_pack(eng, idx, val, bounds):
    """The engine's round-1 construction, verbatim."""
    P = bounds.numel() - 1
    if P > 1:
        split = torch.searchsorted(idx.long(), bounds[1:P]).cpu()
        cuts = [0] + [int(x) for x in split] + [idx.numel()]
    else:
        cuts = [0, idx.numel()]
    counts = [cuts[i + 1] - cuts[i] for i in range(P)]
    segs = [eng._pack(idx[cuts[i]:cuts[i + 1]], val[cuts[i]:cuts[i + 1]])
            for i in range(P)]
    return torch.cat(segs), counts


@pytest.mark.parametrize("wire_bf16", WIRES)
@pytest.mark.parametrize("P,m", SHAPES)
def test_pack_regions_equals_host_construction(P, m, wire_bf16):
    n = max(4 * m, 2 * P, 16)
    idx, val = selection(m, n, seed=17 * P + m)
    eng = engine(wire_bf16)
    for name, bounds in boundary_tables(P, idx, n).items():
        want, want_counts = host_pack(eng, idx, val, bounds)
        for fn in (R.pack_regions, ops.pack_regions):
            got, counts = fn(idx, val, bounds, wire_bf16)
            assert counts == want_counts, (name, counts, want_counts)
            assert got.dtype == torch.int32
            assert torch.equal(got, want), name
            assert got.numel() == sum(eng._pack_ints(c) for c in counts)
        if name == "on_index":  # the boundary index went to the upper region
            k = int((idx < bounds[1]).sum())
            assert want_counts[0] == k and sum(want_counts) == m


def test_pack_regions_odd_segment_pad_is_zero():
    idx = torch.arange(6, dtype=torch.int32)
    val = torch.full((6,), -1.5)
    bounds = torch.tensor([0, 3, 6], dtype=torch.int64)
    buf, counts = R.pack_regions(idx, val, bounds, True)
    assert counts == [3, 3] and buf.numel() == 10
    for seg in (buf[0:5], buf[5:10]):
        halves = seg[3:].view(torch.int16)
        assert halves[3] == 0 and (halves[:3] != 0).all()


@pytest.mark.parametrize("wire_bf16", WIRES)
@pytest.mark.parametrize("P,m", SHAPES)
def test_round_trip(P, m, wire_bf16):
    n = max(4 * m, 2 * P, 16)
    idx, val = selection(m, n, seed=5 * P + m)
    for name, bounds in boundary_tables(P, idx, n).items():
        buf, counts = R.pack_regions(idx, val, bounds, wire_bf16)
        eng = engine(wire_bf16)
        for fn in (R.unpack_segments, ops.unpack_segments):
            r_idx, r_val = fn(buf, counts, wire_bf16)
            h_idx, h_val = eng._unpack(buf, counts)
            assert r_idx.dtype == torch.int32 and r_val.dtype == torch.float32
            assert torch.equal(r_idx, idx), name
            want = val.bfloat16().float() if wire_bf16 else val
            assert torch.equal(r_val.view(torch.int32), want.view(torch.int32)), name
            assert torch.equal(r_idx, h_idx)
            assert torch.equal(r_val.view(torch.int32), h_val.view(torch.int32))


@pytest.mark.parametrize("wire_bf16", WIRES)
@pytest.mark.parametrize("P,m", SHAPES)
def test_unpack_scatter_add_equals_host_path(P, m, wire_bf16):
    """P senders' segments into one owned region [base, base + size)."""
    base, size = 1000, max(2 * m, 8)
    g = torch.Generator().manual_seed(3 * P + m)
    eng = engine(wire_bf16)
    segs, counts = [], []
    for j in range(P):
        c = m if j % 2 == 0 else m // 2  # uneven, some empty when m is small
        i = (torch.randperm(size, generator=g)[:c].sort().values + base).to(torch.int32)
        segs.append(eng._pack(i, torch.randn(c, generator=g)))
        counts.append(c)
    buf = torch.cat(segs)
    want = torch.randn(size, generator=g)
    start = want.clone()
    r_idx, r_val = eng._unpack(buf, counts)
    if r_idx.numel():
        ops.scatter_add_(want, r_idx - base, r_val)
    for fn in (R.unpack_scatter_add_, ops.unpack_scatter_add_):
        got = start.clone()
        out = fn(got, buf, counts, base, wire_bf16)
        assert out is got
        assert torch.equal(got, want)


def test_empty_inputs():
    bounds = torch.tensor([0, 10, 20], dtype=torch.int64)
    e_i = torch.empty(0, dtype=torch.int32)
    e_v = torch.empty(0)
    for wire_bf16 in WIRES:
        buf, counts = ops.pack_regions(e_i, e_v, bounds, wire_bf16)
        assert buf.numel() == 0 and buf.dtype == torch.int32 and counts == [0, 0]
        i, v = ops.unpack_segments(buf, counts, wire_bf16)
        assert i.numel() == 0 and v.numel() == 0
        assert i.dtype == torch.int32 and v.dtype == torch.float32
        dest = torch.ones(5)
        ops.unpack_scatter_add_(dest, buf, counts, 0, wire_bf16)
        assert torch.equal(dest, torch.ones(5))


def test_config_field_defaults_off():
    from oktopk_amd.config import OkTopkConfig

    assert OkTopkConfig().device_wire is False
    cfg = EngineConfig.preset("bert", device_wire=True)
    assert cfg.oktopk.device_wire is True


def test_train_cli_flag():
    from oktopk_amd.train import build_argparser

    assert build_argparser().parse_args([]).device_wire is False
    assert build_argparser().parse_args(["--device-wire"]).device_wire is True


# -- engine equivalence over gloo ---------------------------------------

N = 20_000
DENSITY = 0.01
ITERS = 6


def _grad(rank, it, salt=0):
    g = torch.Generator().manual_seed(1000 * rank + it + 100_000 * salt)
    return torch.randn(N, generator=g)


def _engine_equivalence(rank):
    import torch.distributed as dist

    from oktopk_amd.config import OkTopkConfig

    def build(wire, device_wire):
        return AllReducer(Comm(dist.group.WORLD), EngineConfig(
            compressor="oktopk", density=DENSITY, wire_dtype=wire,
            oktopk=OkTopkConfig(dense_warmup_iters=1,
                                region_repartition_interval=3,
                                device_wire=device_wire)))

    for wire in ("fp32", "bf16"):
        # plain run()
        host, dev = build(wire, False), build(wire, True)
        for it in range(ITERS):
            a = host.run("w", _grad(rank, it))
            b = dev.run("w", _grad(rank, it))
            assert torch.equal(a, b), (wire, it, (a - b).abs().max())
            assert torch.equal(host.states["w"].residual,
                               dev.states["w"].residual), (wire, it)
        # run_many: a batch of 3 tensors through the stage pipeline
        host, dev = build(wire, False), build(wire, True)
        for it in range(ITERS):
            ta = [_grad(rank, it, salt=s) for s in range(3)]
            tb = [t.clone() for t in ta]
            host.run_many([(f"b{s}", ta[s], None) for s in range(3)])
            dev.run_many([(f"b{s}", tb[s], None) for s in range(3)])
            for s in range(3):
                assert torch.equal(ta[s], tb[s]), (wire, it, s)
                assert torch.equal(host.states[f"b{s}"].residual,
                                   dev.states[f"b{s}"].residual), (wire, it, s)


@pytest.mark.parametrize("world", [2, 3])
def test_engine_device_wire_equals_host_path(world):
    run_dist(_engine_equivalence, world)
