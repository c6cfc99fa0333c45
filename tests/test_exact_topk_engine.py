"""EngineConfig.device_exact_topk: topkA / topkA2 / gtopk through
ops.topk_select_ef, ops.topk_select and ops.sparse_merge_topk must give the
same results and residuals, bit for bit, as the torch.topk composition.

torch.topk leaves the choice inside a tie class unspecified, so every
restored tensor a rank selects from is first checked to have distinct k-th
and (k+1)-th magnitudes — a seed that fails the guard is a flaw in the input
and gets replaced, not tolerated.  bf16 gradients alone are coarse (8
significant bits: at k = 163 of 8192 normal samples several share each bf16
value, on one rank and across the ranks a merge compares), so the bf16 runs
start with one fp32 step that leaves a fine-grained fp32 residual; the six
bf16 steps then restore bf16 + fp32 sums, which are apart."""
import pytest
import torch

from conftest import run_dist

N = 8192
DENSITY = 0.02
SEED = 5
ITERS = 6
COMPS = ("gtopk", "topkA", "topkA2")


def _grad(rank, it, n=N):
    g = torch.Generator().manual_seed(7000 * rank + 13 * it + SEED)
    return torch.randn(n, generator=g)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _engine(comp, flag):
    import torch.distributed as dist

    from oktopk_amd import AllReducer, Comm, EngineConfig
    from oktopk_amd.config import OkTopkConfig

    cfg = EngineConfig(compressor=comp, density=DENSITY,
                       device_exact_topk=flag,
                       oktopk=OkTopkConfig(dense_warmup_iters=0))
    return AllReducer(Comm(dist.group.WORLD), cfg)


def _assert_no_tie_at_k(x, k, what):
    mags = torch.sort(x.abs().reshape(-1), descending=True).values
    assert mags[k - 1] != mags[k], f"{what}: tie at the k-th magnitude"


def _flag_on_equals_flag_off(rank, device):
    k = max(1, int(N * DENSITY))
    for bf16_src in (False, True):
        for comp in COMPS:
            off, on = _engine(comp, False), _engine(comp, True)
            # bf16 runs: iteration -1 is the fp32 step that builds a residual
            for it in range(-1 if bf16_src else 0, ITERS):
                g = _grad(rank, it if it >= 0 else ITERS)
                as_bf16 = bf16_src and it >= 0
                restored = g.bfloat16().float() if as_bf16 else g.clone()
                if "w" in off.states:
                    restored += off.states["w"].residual.cpu()
                _assert_no_tie_at_k(
                    restored, k, f"rank {rank} {comp} bf16={bf16_src} it={it}")
                outs = []
                for eng in (off, on):
                    if as_bf16:
                        t = torch.full((N,), 123.0, device=device)  # stale
                        out = eng.run("w", t, grad_src=g.bfloat16().to(device))
                    else:
                        out = eng.run("w", g.clone().to(device))
                    outs.append(out.clone())
                where = (comp, bf16_src, it)
                assert torch.equal(_bits(outs[0]), _bits(outs[1])), where
                assert torch.equal(_bits(off.states["w"].residual),
                                   _bits(on.states["w"].residual)), where
            assert int((outs[1] != 0).sum()) > 0, comp  # really sparse-reduced
            assert int((outs[1] != 0).sum()) <= 4 * k, comp


@pytest.mark.parametrize("world", [2, 3, 4])
def test_flag_on_bit_equal_to_flag_off_cpu(world):
    run_dist(_flag_on_equals_flag_off, world, args=("cpu",))


def _flag_on_equals_flag_off_gpu(rank):
    torch.cuda.set_device(0)
    _flag_on_equals_flag_off(rank, "cuda")


@pytest.mark.gpu
def test_flag_on_bit_equal_to_flag_off_gpu_world2():
    # world 2 only: topkA's merge is an atomic scatter_add_, whose sum is
    # order-dependent from three contributors up
    run_dist(_flag_on_equals_flag_off_gpu, 2)


def _world1_matches(rank):
    _flag_on_equals_flag_off(rank, "cpu")


def test_flag_on_bit_equal_to_flag_off_world1():
    run_dist(_world1_matches, 1)


BIG_N = 4 << 20


def _gtopk_merge_allocates_nothing_dense(rank):
    torch.cuda.set_device(0)
    eng = _engine("gtopk", True)
    for it in range(2):  # the first step creates the state
        t = _grad(rank, it, BIG_N).cuda()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = eng.run("w", t)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
    k = max(1, int(BIG_N * DENSITY))
    assert 0 < int((out != 0).sum()) <= k
    # one torch.zeros(n) of the dense merge alone would add 4n bytes
    assert grown < 4 * BIG_N, (
        f"rank {rank}: step grew device memory by {grown} B, n-sized "
        f"temporary would be {4 * BIG_N} B")


@pytest.mark.gpu
def test_gtopk_flag_on_step_makes_no_n_sized_allocation():
    run_dist(_gtopk_merge_allocates_nothing_dense, 2)
