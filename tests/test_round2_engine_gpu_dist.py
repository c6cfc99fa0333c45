"""OkTopkConfig.device_round2 against the host composition with every rank
computing on cuda:0 (gloo transport): the comparison of
tests/test_round2_tail.py through the HIP kernels, each variant once with
device_wire off and once with it on.

World 3: a round-1 sum of three ranks' values depends on the order of the
scatter-add's float atomics, and the two engines each run their own — so
there the two scatter-add ops are replaced by an order-fixed sum for BOTH
engines (a two-term sum, all world 2 has, is the same in either order).
Everything downstream of the reduce, the code under test, runs unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import run_dist
from test_round2_tail import VARIANTS, engine_equivalence

CONFIGS = [(f"{name}/device_wire={dw}", dict(kw, device_wire=dw))
           for name, kw in VARIANTS.items() if name != "device_wire"
           for dw in (False, True)]


def _worker(rank, fixed_order_reduce):
    from oktopk_amd import ops

    if not fixed_order_reduce:
        return engine_equivalence(rank, "cuda", CONFIGS)

    def scatter_add_(dest, idx, val):
        d = dest.cpu()
        d.index_add_(0, idx.cpu().long(), val.cpu())  # sequential: list order
        return dest.copy_(d)

    def unpack_scatter_add_(dest, buf, counts, base, wire_bf16):
        idx, val = ops.unpack_segments(buf, counts, wire_bf16)
        return scatter_add_(dest, idx - int(base), val)

    saved = ops.scatter_add_, ops.unpack_scatter_add_
    ops.scatter_add_, ops.unpack_scatter_add_ = scatter_add_, unpack_scatter_add_
    try:
        engine_equivalence(rank, "cuda", CONFIGS)
    finally:
        ops.scatter_add_, ops.unpack_scatter_add_ = saved


def test_gpu_world2_device_round2_equals_host_composition():
    run_dist(_worker, 2, args=(False,))


def test_gpu_world3_device_round2_equals_host_composition():
    run_dist(_worker, 3, args=(True,))
