"""OkTopkConfig.device_reduce against the scatter-add composition with every
rank computing on cuda:0 (gloo transport): the comparison of
tests/test_reduce_merge.py through the HIP kernels.

World 2: a two-term sum is the same in either order, so the flag-off engine
runs its float atomics as they are.

World 3: the flag-off engine's two scatter-add ops are replaced by an
order-fixed host sum — the only way its result is defined at all — while the
flag-on engine runs unpatched and must give those bits; and two fresh flag-on
engines fed the same gradients must agree with each other bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import run_dist
from test_reduce_merge import (CONFIGS, ITERS, assert_same_state, build_engine,
                               engine_equivalence, engine_grad, same_bits)


def _ordered_scatter_adds(ops):
    """(scatter_add_, unpack_scatter_add_) summing on the host in list order."""

    def scatter_add_(dest, idx, val):
        d = dest.cpu()
        d.index_add_(0, idx.cpu().long(), val.cpu())  # sequential: list order
        return dest.copy_(d)

    def unpack_scatter_add_(dest, buf, counts, base, wire_bf16):
        idx, val = ops.unpack_segments(buf, counts, wire_bf16)
        return scatter_add_(dest, idx - int(base), val)

    return scatter_add_, unpack_scatter_add_


def _world2(rank):
    engine_equivalence(rank, "cuda", CONFIGS, 2)


def _world3(rank):
    from oktopk_amd import ops

    saved = ops.scatter_add_, ops.unpack_scatter_add_
    ops.scatter_add_, ops.unpack_scatter_add_ = _ordered_scatter_adds(ops)
    try:
        # only the flag-off engine ever reaches the two patched ops
        engine_equivalence(rank, "cuda", CONFIGS, 3)
    finally:
        ops.scatter_add_, ops.unpack_scatter_add_ = saved

    # run-to-run: two fresh flagged engines, nothing patched
    for label, kw in CONFIGS:
        one, two = build_engine(True, kw), build_engine(True, kw)
        for it in range(ITERS):
            t = engine_grad(rank, it).cuda()
            a = one.run("w", t.clone())
            b = two.run("w", t.clone())
            assert same_bits(a, b), (label, it)
            assert_same_state(one, two, (label, it))


def test_gpu_world2_device_reduce_equals_scatter_add_composition():
    run_dist(_world2, 2)


def test_gpu_world3_device_reduce_is_ordered_and_reproducible():
    run_dist(_world3, 3)
