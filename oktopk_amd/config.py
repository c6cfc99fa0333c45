"""Typed configuration for the Ok-Topk MI355X engine.

The reference hard-codes its cadence/tuning constants inside the allreducer
(/root/reference/VGG/allreducer.py:27,209-211,573-582,673 and
/root/reference/BERT/bert/allreducer.py:355-361,412).  Here every knob lives in
one dataclass so workload recipes (VGG / LSTM / BERT) are plain config presets
instead of three forked source trees.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field


@dataclass
class OkTopkConfig:
    """Cadence + feedback-controller constants of the Ok-Topk algorithm.

    Defaults follow the VGG recipe of the reference
    (/root/reference/VGG/allreducer.py:573-582), with the throttle lifted to 7
    to match one in-flight peer per xGMI link on MI355X (the reference used 4
    for Cray Aries, /root/reference/VGG/allreducer.py:673).
    """

    # Iterations of dense warm-up allreduce before sparsification kicks in
    # (512 VGG / 128 LSTM / 0 BERT in the reference).
    dense_warmup_iters: int = 512
    # Exact top-k threshold recompute cadence (local selection).
    local_threshold_recompute_interval: int = 32
    # Exact global top-k recompute cadence (round 2).
    global_threshold_recompute_interval: int = 32
    # Balanced index-range repartition cadence.
    region_repartition_interval: int = 64
    # Feedback-controller scales (reference /root/reference/VGG/allreducer.py:209-211).
    scale_local: float = 1.012
    scale_global_increase: float = 1.008
    scale_global_decrease: float = 1.008
    # add2residual adaptive bump (reference VGG/compression.py:244-255).
    bump_scale: float = 1.03
    bump_max_loops: int = 5
    # Local feedback bounds: shrink tau if selected < lo_frac*k, grow if > hi_frac*k
    # (2/3 and 5/4 in the reference, VGG/allreducer.py:696-699).
    local_lo_num: int = 2
    local_lo_den: int = 3
    local_hi_num: int = 5
    local_hi_den: int = 4
    # Global feedback bounds (2/3 and 4/3, VGG/allreducer.py:1054-1057).
    global_lo_num: int = 2
    global_lo_den: int = 3
    global_hi_num: int = 4
    global_hi_den: int = 3
    # Chunked engine pipeline (docs/overlap_design.md): split the flat
    # gradient into this many slices, each with independent thresholds /
    # regions / residual (the VGG reference's per-group processing), and
    # interleave the stages so chunk i's collectives overlap chunk i+1's
    # compress on RCCL.  1 = the plain single-pass engine (default; flip
    # only after the 8-GPU win is measured).
    pipeline_chunks: int = 1
    # Round-2 load-balanced redistribution (reference
    # BERT/bert/allreducer.py:615-715): re-balance the per-owner survivors
    # into equal ceil(S/P) blocks with one alltoallv, then exchange with a
    # single perfectly-equal AllGather — wire volume S+pad instead of
    # P*max(s_r).  Pays when region survivor counts are skewed; the default
    # pad-to-max path is one collective fewer.
    balanced_allgather: bool = False
    # Device-side wire codec: round 1 packs the per-destination segments
    # with ops.pack_regions (two launches + the one count readback, in
    # place of searchsorted + P slice-packs + cat), reduces the received
    # payload with ops.unpack_scatter_add_ (one launch, nothing unpacked
    # into temporaries), and round 2 unpacks with ops.unpack_segments.
    # Same wire bytes as the host path.  Kernel-level timings against the
    # host path are in profiles/README.md; whether it shortens a real
    # multi-GPU step is unmeasured (default off; flip only after the
    # multi-GPU win is measured).
    device_wire: bool = False
    # Device-side round-2 tail: everything after the sparse allgather —
    # the global selection (every gathered entry, or on an exact-recompute
    # iteration the k of largest magnitude) and the residual credit — is
    # one ops.round2_tail_ / ops.round2_tail_wire_ call, in place of
    # abs + torch.topk + .item() + two gathers and the n-element bool mask
    # with its two index_puts.  The wire form (with device_wire, after the
    # plain allgather) decodes the gathered buffer in the same kernel.  The
    # selection comes back ascending on every iteration, so the sparse
    # hand-over to clip / Adam also covers the exact iterations and
    # balanced_allgather; TensorState.mask is never allocated.  Ties at the
    # k-th magnitude go to the lowest gathered position where torch.topk
    # leaves the choice unspecified.  Kernel-level timings against the torch
    # composition are in profiles/README.md; whether it shortens a real
    # multi-GPU step is unmeasured (default off; flip only after the
    # multi-GPU win is measured).
    device_round2: bool = False
    # Device-side round-1 reduce: at a region owner the received payload —
    # P rank-ordered, ascending segments — is reduced by one
    # ops.reduce_segments / ops.reduce_segments_wire call (a P-way merge of
    # sorted runs with the threshold filter folded in), in place of
    # zeros(hi - lo) + scatter_add_ / unpack_scatter_add_ + compact_gt +
    # "+ lo".  The wire form (with device_wire) decodes the received buffer
    # in the same kernels.  Work is sized by the payload, the dense region
    # is never allocated, and no float atomic runs: an index with three or
    # more contributors sums in rank order, as the CPU reference does, so a
    # world >= 3 step is bit-reproducible.  World 1 has no reduce and is
    # untouched.  Kernel-level timings against the scatter-add composition
    # are in profiles/README.md; whether it shortens a real multi-GPU step
    # is unmeasured (default off; flip only after the multi-GPU win is
    # measured).
    device_reduce: bool = False


@dataclass
class EngineConfig:
    """Engine-wide configuration."""

    compressor: str = "oktopk"
    density: float = 0.001
    # per-epoch density schedule (reference _dynamic_densities,
    # VGG/allreducer.py:265-270): density used = schedule[min(epoch, len-1)]
    # when non-empty, else `density`
    dynamic_densities: tuple = ()
    # Gradient-bucket merge threshold in bytes (reference groups at 640 MB,
    # /root/reference/VGG/allreducer.py:27; we default far smaller because
    # xGMI-chunked RCCL likes a handful of large-but-not-huge buckets).
    bucket_bytes: int = 64 << 20
    # dtype used on the wire for sparse values ("fp32" | "bf16").
    wire_dtype: str = "fp32"
    oktopk: OkTopkConfig = field(default_factory=OkTopkConfig)
    # Device-resident selection for gaussiank / gaussiankconcat /
    # gaussiankSA: one ops.gaussian_select_ef call (EF restore with fused
    # fp64 moments, on-device normal quantile, one 10-candidate count pass,
    # on-device refine walk, compact write; one 48-byte readback) in place
    # of the EF restore + torch mean/std + scipy ppf + up to three count_gt
    # rounds + compact_gt (+ the residual copy of gaussiank).  With it on,
    # gaussiank / gaussiankconcat also take the fused bf16 grad_src upcast.
    # tau0 comes from fp64 moments rounded once to fp32, so tau can differ
    # from the host path (fp32 moments, double tau) in the last bits — and
    # the selection with it when an element sits exactly there.  Kernel-
    # level timings against the host composition are in profiles/README.md;
    # default off until a multi-GPU step time is measured.
    gaussian_device_select: bool = False
    # Device-resident exact top-k for topkA / topkA2 / gtopk: the local
    # selection is one ops.topk_select_ef call (EF restore with the first
    # radix-histogram level fused in, two more levels, a (gt, eq) count and
    # an ascending write that also zeroes the residual; one 16-byte
    # readback) in place of add_ + torch.topk + gather + residual copy +
    # zero_at_; topkA2's second truncation is ops.topk_select; each gtopk
    # tree round merges with ops.sparse_merge_topk (work sized by the two
    # k-entry packets) in place of zeros(n) + two scatters + torch.topk over
    # n.  With it on, the three modes also take the fused bf16 grad_src
    # upcast.  Same wire format, packet size and tree schedule; ties at the
    # k-th magnitude go to the lowest index where torch.topk leaves the
    # choice unspecified.  Kernel-level timings against the torch
    # composition are in profiles/README.md; whether it shortens a real
    # multi-GPU step is unmeasured (default off; flip only after the
    # multi-GPU win is measured).
    device_exact_topk: bool = False
    # EPS oracle (reference settings.PROFILING_NORM): when on, a dense
    # allreduce runs alongside the sparse one and the relative L2 error of the
    # sparse result is recorded.
    profiling_norm: bool = False
    # Per-phase timing table cadence (reference prints every 50 iterations).
    profiling: bool = False
    profiling_interval: int = 50
    # gradient-distribution research dumps (reference PROFILING_GRAD,
    # VGG/allreducer.py:608-623): save |grad| histograms + thresholds for
    # the named iterations into profiling_grad_dir
    profiling_grad_iters: tuple = ()
    profiling_grad_dir: str = "grad_dumps"

    @classmethod
    def preset(cls, name: str, **overrides) -> "EngineConfig":
        """Workload presets mirroring the reference's three tunings."""
        if name == "vgg":
            cfg = cls(oktopk=OkTopkConfig())
        elif name == "lstm":
            cfg = cls(
                oktopk=OkTopkConfig(
                    dense_warmup_iters=128,
                    scale_local=1.01,
                    local_lo_num=3,
                    local_lo_den=4,
                )
            )
        elif name == "bert":
            cfg = cls(
                oktopk=OkTopkConfig(
                    dense_warmup_iters=0,
                    local_threshold_recompute_interval=128,
                    global_threshold_recompute_interval=128,
                    region_repartition_interval=64,
                    local_lo_num=4,
                    local_lo_den=5,
                )
            )
        else:
            raise ValueError(f"unknown preset {name!r}")
        for k, v in overrides.items():
            if hasattr(cfg, k):
                setattr(cfg, k, v)
            elif hasattr(cfg.oktopk, k):
                setattr(cfg.oktopk, k, v)
            else:
                raise AttributeError(f"no config field {k!r}")
        return cfg

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)
