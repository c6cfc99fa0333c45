#!/usr/bin/env python3
"""Microbenchmark of every HIP op at BERT-base flat-gradient scale (109.5M
fp32).  Reports ms and effective HBM GB/s against the op's algorithmic byte
count; run under rocprofv3 --pmc for counter confirmation."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oktopk_amd import _hip_ops as H

N = 109_500_000
GB = 1e9


def timeit(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def timeit_graph(fn, reps=100, replays=5):
    """For microsecond-scale kernels: `reps` back-to-back calls captured
    into one hipGraph, so the host's launch cost does not set the floor.
    Seconds per call, kernel boundary (~1.5 us) included — what one such
    kernel costs inside the captured fwd+bwd."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * replays)


def colsum_rows():
    """Bias-gradient column sum at the BERT-base shapes: the two one-launch
    kernels that store into an (unaligned) gradient slot (colsum_into: own
    order; colsum_exact: torch's order, torch's bits) vs torch's sum(0) into
    a preallocated output."""
    g = torch.Generator().manual_seed(1)
    rows = []
    for C in (768, 2304, 3072, 30522):
        gy = torch.randn(1024, C, generator=g).bfloat16().cuda()
        dst = torch.empty(C + 8, dtype=torch.bfloat16, device="cuda")[3:3 + C]
        out = torch.empty(C, dtype=torch.bfloat16, device="cuda")
        nbytes = 2 * 1024 * C
        for name, fn in (
            (f"colsum_into [1024,{C}]", lambda: H.colsum_bf16_into(gy, dst, False)),
            (f"colsum_exact [1024,{C}]",
             lambda: H.colsum_bf16_into_exact(gy, dst, False)),
            (f"torch sum(0) [1024,{C}]", lambda: torch.sum(gy, 0, out=out)),
        ):
            ms = timeit_graph(fn) * 1000
            rows.append((name, ms, nbytes / GB / (ms / 1000)))
    return rows


def time_both(fn, iters, warmup=5):
    """(device us, host wall us) per call over one window of `iters` calls.
    Wall: host clock around the window, ending in a device synchronise.
    Device: events bracketing the same window — the span the call occupies
    on the GPU timeline, gaps where the device waits for the host's next
    launch included (that is what a serial engine step pays)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / iters
    return e0.elapsed_time(e1) * 1000 / iters, wall * 1e6


def wire_rows(iters):
    """Sparse wire codec (ops/csrc/wire_codec.hip) against the engine's host
    path, same run, same inputs: m ~ 110k selected entries (BERT-base at
    density 0.1%), P = 2 / 8 / 64 regions, fp32 and bf16 wire.

      pack     ops.pack_regions  vs  searchsorted + .cpu() + P x _pack + cat
      reduce   ops.unpack_scatter_add_  vs  _unpack + (idx - lo) + scatter_add_
               (the payload one owner receives: P segments of ~m/P entries)
      unpack   ops.unpack_segments  vs  _unpack   (round-2 allgather result)
    Outputs of the two paths are compared before anything is timed."""
    from oktopk_amd import AllReducer, Comm, EngineConfig, ops

    n, m = 109_500_000, 110_000
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, n, (2 * m,), generator=g).unique()  # ascending
    idx = idx[torch.randperm(idx.numel(), generator=g)[:m].sort().values]
    idx = idx.to(torch.int32).cuda()
    val = torch.randn(m, generator=g).cuda()
    rows = []
    for P in (2, 8, 64):
        bounds = torch.tensor([i * (n // P) for i in range(P)] + [n],
                              dtype=torch.int64)
        for wire in ("fp32", "bf16"):
            bf = wire == "bf16"
            eng = AllReducer(Comm(None), EngineConfig(wire_dtype=wire))

            def host_pack():
                sp = torch.searchsorted(idx.long(), bounds[1:P].to(idx.device)).cpu()
                cuts = [0] + [int(x) for x in sp] + [m]
                return torch.cat([eng._pack(idx[cuts[i]:cuts[i + 1]],
                                            val[cuts[i]:cuts[i + 1]])
                                  for i in range(P)]), cuts

            send, cuts = host_pack()
            dsend, counts = ops.pack_regions(idx, val, bounds, bf)
            assert torch.equal(send, dsend)
            assert counts == [cuts[i + 1] - cuts[i] for i in range(P)]
            # the payload the owner of region 0 receives: P senders' region-0
            # segments (the same segment P times — duplicates hit every slot)
            lo, hi = 0, int(bounds[1])
            recv = send[:eng._pack_ints(counts[0])].repeat(P)
            rc = [counts[0]] * P
            reduced = torch.zeros(hi - lo, device="cuda")

            def host_reduce():
                r_idx, r_val = eng._unpack(recv, rc)
                ops.scatter_add_(reduced, r_idx - lo, r_val)

            a, b = eng._unpack(recv, rc)
            c, d = ops.unpack_segments(recv, rc, bf)
            assert torch.equal(a, c) and torch.equal(b, d)
            # round-2 shape: P owners' survivor segments, ~m entries in all
            gathered, gc = send, counts
            for name, fn in (
                (f"pack    host   P={P} {wire}", host_pack),
                (f"pack    device P={P} {wire}",
                 lambda: ops.pack_regions(idx, val, bounds, bf)),
                (f"reduce  host   P={P} {wire}", host_reduce),
                (f"reduce  device P={P} {wire}",
                 lambda: ops.unpack_scatter_add_(reduced, recv, rc, lo, bf)),
                (f"unpack  host   P={P} {wire}",
                 lambda: eng._unpack(gathered, gc)),
                (f"unpack  device P={P} {wire}",
                 lambda: ops.unpack_segments(gathered, gc, bf)),
            ):
                dev_us, wall_us = time_both(fn, iters)
                rows.append((name, dev_us, wall_us))
    print(f"# wire codec, m={m} entries, index space n={n}, {iters} calls/row")
    print(f"{'path':30s} {'device us':>10s} {'wall us':>10s}")
    for name, dev_us, wall_us in rows:
        print(f"{name:30s} {dev_us:10.1f} {wall_us:10.1f}")


def gauss_rows(reps, sizes=(109_500_000, 25_000_000), density=0.001,
               device="cuda"):
    """Device-resident Gaussian-k selection (ops.gaussian_select_ef,
    ops/csrc/gauss_select.hip) against the host composition the gaussiank
    engine path runs without it: ef_restore_snapshot_ + _gaussian_threshold
    (torch mean/std + scipy ppf) + the three-round count_gt loop +
    compact_gt + residual.copy_.  Inputs: randn (the loop stops at round 1)
    and randn**3 (all three rounds).  Both paths end in a host readback, so
    each call is timed alone: reset inputs, synchronise, host clock around
    call + synchronise.  The two paths alternate inside one repeat loop;
    median and min..max over `reps` repeats."""
    from oktopk_amd import ops
    from oktopk_amd.allreducer import _gaussian_threshold

    def sync():
        if device != "cpu":
            torch.cuda.synchronize()

    print(f"# gaussian select, density={density}, {reps} repeats/row")
    print(f"{'path':34s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s}")
    for n in sizes:
        k = max(1, int(n * density))
        g = torch.Generator().manual_seed(0)
        x = torch.randn(n, generator=g)
        r0 = (torch.randn(n, generator=g) * 0.01).to(device)
        for label, t0 in (("randn", x.to(device)), ("randn**3", (x ** 3).to(device))):
            t, r = t0.clone(), r0.clone()

            def host():
                ops.ef_restore_snapshot_(t, r)
                tau = _gaussian_threshold(t, density)
                for _ in range(3):
                    cnt = ops.count_gt(t, tau)
                    if cnt < 2 * k / 3:
                        tau *= 0.5
                    elif cnt > 4 * k / 3:
                        tau *= 1.5
                    else:
                        break
                idx, val = ops.compact_gt(t, tau)
                r.copy_(t)
                return idx, tau

            def dev():
                out = ops.gaussian_select_ef(t, r, None, density, k)
                return out[0], out[4]

            times = {"host": [], "device": []}
            sel = {}
            for rep in range(reps + 2):  # two warm-up repeats
                for name, fn in (("host", host), ("device", dev)):
                    t.copy_(t0)
                    r.copy_(r0)
                    sync()
                    c0 = time.perf_counter()
                    idx, tau = fn()
                    sync()
                    if rep >= 2:
                        times[name].append((time.perf_counter() - c0) * 1000)
                    sel[name] = (idx.numel(), tau)
            # same decision (tau may differ in the last bits: fp32 vs fp64
            # moments), so the selected counts agree to a few elements
            assert abs(sel["host"][1] - sel["device"][1]) <= 1e-4 * sel["host"][1], sel
            assert abs(sel["host"][0] - sel["device"][0]) <= 0.01 * k + 2, sel
            for name in ("host", "device"):
                ts = sorted(times[name])
                print(f"{name:6s} {label:9s} n={n:<11d} sel={sel[name][0]:<8d}"
                      f"{ts[len(ts) // 2]:10.3f} {ts[0]:9.3f} {ts[-1]:9.3f}")


def _alternate(arms, reset, reps):
    """Each arm timed alone (reset, synchronise, host clock around call +
    synchronise), the arms alternating inside one repeat loop; two warm-up
    repeats.  Returns {name: sorted ms} and {name: last result}."""
    times = {name: [] for name, _ in arms}
    last = {}
    for r in range(reps + 2):
        for name, fn in arms:
            reset()
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((time.perf_counter() - c0) * 1000)
    return {k: sorted(v) for k, v in times.items()}, last


def topk_rows(reps, sizes=(109_500_000, 336_000_000), density=0.001):
    """Exact top-k ops (ops/csrc/topk_select.hip) against the torch
    compositions the topkA / gtopk engine paths run without
    device_exact_topk.  Select: add_ + torch.topk(|t|, k) + gather +
    residual.copy_ + zero_at_ (plus the bf16 upcast copy_ in the bf16 rows)
    against one topk_select_ef.  Merge: zeros(n) + two scatter_add_ +
    torch.topk over n + gather against sparse_merge_topk on the two k-entry
    packets.  Every arm ends in a host readback or an allocation, so each
    call is timed alone; median and min..max over `reps` repeats."""
    from oktopk_amd import ops

    print(f"# exact top-k, density={density}, {reps} repeats/row")
    print(f"{'path':44s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s}")

    def show(label, n, ts):
        print(f"{label:30s} n={n:<11d} {ts[len(ts) // 2]:10.3f} "
              f"{ts[0]:9.3f} {ts[-1]:9.3f}")

    def same_magnitudes(last):
        # torch.topk may pick other members of the tie class at the k-th
        # magnitude; the selected magnitudes are the same either way
        a, b = (last[x][1].abs().sort().values for x in ("torch", "hip"))
        assert torch.equal(a, b), "selections differ"

    for n in sizes:
        k = max(1, int(n * density))
        g = torch.Generator(device="cuda").manual_seed(0)
        t0 = torch.randn(n, device="cuda", generator=g)
        r0 = torch.randn(n, device="cuda", generator=g) * 0.1
        g16 = t0.to(torch.bfloat16)
        t, r = t0.clone(), r0.clone()

        def reset():
            t.copy_(t0)
            r.copy_(r0)

        def torch_select(grad):
            if grad is not None:
                t.copy_(grad.to(t.dtype))
            t.add_(r)
            topv = torch.topk(t.abs(), k, sorted=False)
            idx = topv.indices.to(torch.int32)
            val = t[topv.indices]
            r.copy_(t)
            ops.zero_at_(r, idx)
            return idx, val

        for tag, grad in (("fp32", None), ("bf16", g16)):
            times, last = _alternate(
                (("torch", lambda: torch_select(grad)),
                 ("hip", lambda: ops.topk_select_ef(t, r, grad, k)[:2])),
                reset, reps)
            same_magnitudes(last)
            show(f"select {tag} torch 5-op", n, times["torch"])
            show(f"select {tag} topk_select_ef", n, times["hip"])

        a_idx, a_val, _ = ops.topk_select(t0, k)
        b_idx, b_val, _ = ops.topk_select(r0, k)

        def dense_merge():
            merged = torch.zeros(n, dtype=t0.dtype, device="cuda")
            ops.scatter_add_(merged, a_idx, a_val)
            ops.scatter_add_(merged, b_idx, b_val)
            topm = torch.topk(merged.abs(), k, sorted=False)
            return topm.indices.to(torch.int32), merged[topm.indices]

        times, last = _alternate(
            (("torch", dense_merge),
             ("hip", lambda: ops.sparse_merge_topk(a_idx, a_val, b_idx, b_val, k))),
            lambda: None, reps)
        same_magnitudes(last)
        show("merge dense zeros+scatter+topk", n, times["torch"])
        show("merge sparse_merge_topk", n, times["hip"])
        del t0, r0, g16, t, r


def round2_rows(reps, sizes=(109_500_000, 336_000_000), density=0.001, P=8):
    """Ok-Topk round-2 tail (ops/csrc/round2_tail.hip) against the torch
    composition the engine runs without device_round2, same process, same
    inputs, arms alternating: ops.unpack_segments, then on an exact
    iteration abs + torch.topk(sorted=True) + .item() + two gathers, then
    the residual credit through the persistent n-element bool mask (two
    int64 index copies, two index_puts, zero_at_masked_) — against one
    ops.round2_tail_wire_ call on the gathered buffer.  BERT-base and
    BERT-large flat sizes at density 0.1 %, gathered S = 4k/3 and 4k entries
    in 8 segments, fp32 and bf16 wire, threshold (k=None) and exact mode;
    the local selection holds ~k entries, half of them gathered ones.  Each
    call is timed alone; median and min..max over `reps` repeats."""
    from oktopk_amd import ops

    print(f"# round-2 tail, density={density}, P={P} segments, "
          f"{reps} repeats/row")
    print(f"{'path':58s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s}")
    for n in sizes:
        k = max(1, int(n * density))
        g = torch.Generator().manual_seed(0)
        residual = torch.full((n,), 0.5, device="cuda")
        mask = torch.zeros(n, dtype=torch.bool, device="cuda")
        print(f"# n={n} k={k}: mask bytes the flag no longer allocates = {n}")
        for S in (4 * k // 3, 4 * k):
            pool = torch.randint(0, n, (2 * S + 2 * k,), generator=g).unique()
            pool = pool[torch.randperm(pool.numel(), generator=g)]
            all_idx = pool[:S].sort().values.to(torch.int32).cuda()
            # local selection: k/2 gathered entries + k/2 others
            idx = torch.cat([pool[:k // 2], pool[S:S + k - k // 2]]) \
                .sort().values.to(torch.int32).cuda()
            bounds = torch.tensor([i * (n // P) for i in range(P)] + [n],
                                  dtype=torch.int64)
            for wire in ("fp32", "bf16"):
                bf = wire == "bf16"
                val = torch.randn(S, generator=g).cuda()
                buf, counts = ops.pack_regions(all_idx, val, bounds, bf)

                def torch_tail(kk):
                    a_idx, a_val = ops.unpack_segments(buf, counts, bf)
                    tau = None
                    if kk is not None:
                        top = torch.topk(a_val.abs(), min(kk, a_val.numel()),
                                         sorted=True)
                        tau = float(top.values[-1].item())
                        a_idx, a_val = a_idx[top.indices], a_val[top.indices]
                    mask[a_idx.long()] = True
                    ops.zero_at_masked_(residual, idx, mask)
                    mask[a_idx.long()] = False
                    return a_idx, a_val, tau

                for mode, kk in (("threshold", None), ("exact", k)):
                    times, last = _alternate(
                        (("torch", lambda: torch_tail(kk)),
                         ("hip", lambda: ops.round2_tail_wire_(
                             residual, idx, buf, counts, bf, kk))),
                        lambda: None, reps)
                    # torch.topk may pick other members of the tie class at
                    # the k-th magnitude (bf16 values tie): same magnitudes,
                    # same tau
                    a, b = (last[x][1].abs().sort().values
                            for x in ("torch", "hip"))
                    assert torch.equal(a, b), "selections differ"
                    assert last["torch"][2] == last["hip"][2]
                    for arm, label in (("torch", "torch unpack+topk+mask"),
                                       ("hip", "round2_tail_wire_")):
                        ts = times[arm]
                        print(f"{mode:9s} {wire} S={S:<8d} n={n:<10d} "
                              f"{label:24s} {ts[len(ts) // 2]:10.3f} "
                              f"{ts[0]:9.3f} {ts[-1]:9.3f}")
        del residual, mask


def reduce_rows(reps, sizes=(109_500_000, 336_000_000), worlds=(2, 8, 64),
                densities=(0.001, 0.01)):
    """Ok-Topk round-1 reduce at a region owner (ops/csrc/reduce_merge.hip)
    against the composition the engine runs without device_reduce, same
    process, same inputs, arms alternating: zeros(n / P) + scatter_add_ (pair
    form) or unpack_scatter_add_ (wire form) + compact_gt + "+ lo" — against
    one ops.reduce_segments / ops.reduce_segments_wire call.  BERT-base and
    BERT-large flat sizes, region length n / P, payload P segments of k / P
    entries: each rank holds about half of a shared hot set of k / P region
    indices plus private ones, so runs of every length up to P occur.  Values
    are multiples of 2^-8 (also after the bf16 rounding), so every sum is
    exact and the two arms are compared for equality before timing despite
    the baseline's atomics.  tau = 0 (exact iteration) and tau = 1
    (threshold).  Each call ends in a host readback, so each is timed alone;
    median and min..max over `reps` repeats."""
    from oktopk_amd import ops

    print(f"# round-1 reduce, {reps} repeats/row; M = payload entries, "
          f"kept = survivors")
    print(f"{'path':74s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s}")
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in sizes:
        for density in densities:
            k = max(1, int(n * density))
            for P in worlds:
                length = n // P
                lo = (P // 2) * length
                c = max(1, k // P)
                hot = torch.randperm(length, generator=g, device="cuda")[:c]
                segs = []
                for _ in range(P):
                    mine = hot[torch.rand(c, generator=g, device="cuda") < 0.5]
                    own = torch.randint(0, length, (c - mine.numel(),),
                                        generator=g, device="cuda")
                    segs.append((torch.cat([mine, own]).unique() + lo)
                                .to(torch.int32))
                counts = [int(s.numel()) for s in segs]
                idx = torch.cat(segs)
                M = idx.numel()
                val = torch.randint(-512, 513, (M,), generator=g,
                                    device="cuda").float() / 256
                one = torch.tensor([0, n], dtype=torch.int64)
                forms = [("pair", None, None)]
                for wire in ("fp32", "bf16"):
                    bf = wire == "bf16"
                    parts, off = [], 0
                    for cj in counts:
                        parts.append(ops.pack_regions(
                            idx[off:off + cj], val[off:off + cj], one, bf)[0])
                        off += cj
                    forms.append((wire, torch.cat(parts), bf))

                def scatter_arm(buf, bf, tau):
                    reduced = torch.zeros(length, device="cuda")
                    if buf is None:
                        ops.scatter_add_(reduced, idx - lo, val)
                    else:
                        ops.unpack_scatter_add_(reduced, buf, counts, lo, bf)
                    gi, gv = ops.compact_gt(reduced, tau)
                    return gi + lo, gv

                def merge_arm(buf, bf, tau):
                    if buf is None:
                        return ops.reduce_segments(idx, val, counts, lo, length, tau)
                    return ops.reduce_segments_wire(buf, counts, bf, lo, length, tau)

                for form, buf, bf in forms:
                    for mode, tau in (("exact", 0.0), ("threshold", 1.0)):
                        a = scatter_arm(buf, bf, tau)
                        b = merge_arm(buf, bf, tau)
                        assert torch.equal(a[0], b[0]), "indices differ"
                        assert torch.equal(a[1].view(torch.int32),
                                           b[1].view(torch.int32)), "sums differ"
                        times, _ = _alternate(
                            (("scatter", lambda: scatter_arm(buf, bf, tau)),
                             ("merge", lambda: merge_arm(buf, bf, tau))),
                            lambda: None, reps)
                        for arm, label in (("scatter", "zeros+scatter_add+compact_gt"),
                                           ("merge", "reduce_segments")):
                            ts = times[arm]
                            print(f"{mode:9s} {form:4s} n={n:<10d} P={P:<3d} "
                                  f"M={M:<8d} kept={a[0].numel():<8d} "
                                  f"{label:28s} {ts[len(ts) // 2]:10.3f} "
                                  f"{ts[0]:9.3f} {ts[-1]:9.3f}")
                del segs, idx, val, forms


def sparse_step_rows(iters, density=0.001):
    """The optimizer tail at the 109.5 M flat scale with k = 0.1 %: the dense
    hand-over (zero fill + scatter + dense sum of squares + Adam over p, g,
    m, v and the bf16 mirror) against the sparse pair (grad_clip_scale_sparse
    + fused_adam_sparse_mirror_).  Bytes are the algorithm's, from the
    shapes: Adam reads p, m, v (+g dense) and writes p, m, v and the bf16
    mirror — 30 B/element dense, 26 B/element sparse.  The count readback of
    scatter_gt_credit_ is left out of both arms (credit only through
    zero_at_), so the rows time device work, not the host sync."""
    g = torch.Generator().manual_seed(0)
    k = int(N * density)
    idx = torch.randperm(N, generator=g)[:k].sort().values.to(torch.int32).cuda()
    val = torch.randn(k, generator=g).cuda()
    p = torch.randn(N, generator=g).cuda()
    m = torch.zeros(N, device="cuda")
    v = torch.zeros(N, device="cuda")
    mirror = torch.zeros(N, dtype=torch.bfloat16, device="cuda")
    dense = torch.empty(N, device="cuda")
    adam = (1e-3, 0.9, 0.999, 1e-6, 0.01)
    print(f"# N={N}  entries={k}")

    def dense_tail():
        H.fill_sparse_scaled_(dense, idx, val, 1.0)
        gs = H.grad_clip_scale(dense, 1.0)
        H.fused_adam_mirror_(p, dense, m, v, mirror, *adam, gs)

    def sparse_tail():
        gs = H.grad_clip_scale_sparse(idx, val, 1.0, -1.0, 1.0)
        H.fused_adam_sparse_mirror_(p, idx, val, 0, 1.0, -1.0, m, v, mirror,
                                    *adam, gs)

    gs1 = H.grad_clip_scale_sparse(idx, val, 1.0, -1.0, 1.0)
    rows = []
    for name, fn, nbytes in (
        ("fill_sparse_scaled (zero+scatter)",
         lambda: H.fill_sparse_scaled_(dense, idx, val, 1.0), 4 * N + 12 * k),
        ("grad_clip_scale (dense)",
         lambda: H.grad_clip_scale(dense, 1.0), 4 * N),
        ("adam mirror (dense g)",
         lambda: H.fused_adam_mirror_(p, dense, m, v, mirror, *adam, gs1), 30 * N),
        ("dense tail (all three)", dense_tail, (4 + 4 + 30) * N + 12 * k),
        ("grad_clip_scale_sparse",
         lambda: H.grad_clip_scale_sparse(idx, val, 1.0, -1.0, 1.0), 4 * k),
        ("adam mirror (sparse g)",
         lambda: H.fused_adam_sparse_mirror_(p, idx, val, 0, 1.0, -1.0, m, v,
                                             mirror, *adam, gs1),
         26 * N + 8 * k),
        ("sparse tail (both)", sparse_tail, 26 * N + 12 * k),
    ):
        dev_us, _wall = time_both(fn, iters)
        rows.append((name, dev_us / 1000, nbytes / GB / (dev_us / 1e6)))
    return rows


def flat_sgd_rows(iters, sizes=(15_000_000, 27_000_000), density=0.001,
                  ntensors=60):
    """The SGD tail at the VGG-16 (15 M) and lstman4 (27 M) scales with
    k = 0.1 %: sgd_step_ on a dense gradient, the densify (zero fill +
    scatter) that precedes it, sgd_step_sparse_ on the selection, and
    torch's foreach SGD over the same storage viewed as `ntensors` parameter
    tensors.  momentum 0.9, weight decay 5e-4, no clip.  Bytes are the
    algorithm's, per element: the fused dense step moves 5 streams (20 B),
    the sparse one 4 (16 B, plus 8 B per entry), the fill 4 B; torch's
    step as separate passes g + wd*p (12), buf*mom (8), buf + d (12),
    p - lr*d (12) = 44 B."""
    g = torch.Generator().manual_seed(0)
    rows = []
    for n in sizes:
        k = int(n * density)
        idx = torch.randperm(n, generator=g)[:k].sort().values.to(torch.int32).cuda()
        val = torch.randn(k, generator=g).cuda()
        p = torch.randn(n, generator=g).cuda()
        buf = torch.zeros(n, device="cuda")
        dense = torch.empty(n, device="cuda")
        H.fill_sparse_scaled_(dense, idx, val, 1.0)
        hp = (0.1, 0.9, 5e-4, False)
        cuts = [n * j // ntensors for j in range(ntensors + 1)]
        params = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            q = torch.nn.Parameter(p[a:b])
            q.grad = dense[a:b]
            params.append(q)
        topt = torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4,
                               foreach=True)
        topt.step()  # allocates the momentum buffers

        def torch_route():
            H.fill_sparse_scaled_(dense, idx, val, 1.0)
            topt.step()

        def dense_route():
            H.fill_sparse_scaled_(dense, idx, val, 1.0)
            H.sgd_step_(p, dense, buf, *hp)

        for name, fn, nbytes in (
            (f"sgd_step_ n={n}", lambda: H.sgd_step_(p, dense, buf, *hp), 20 * n),
            (f"fill + sgd_step_ n={n}", dense_route, 24 * n + 12 * k),
            (f"sgd_step_sparse_ n={n}",
             lambda: H.sgd_step_sparse_(p, idx, val, 0, 1.0, -1.0, buf, *hp),
             16 * n + 8 * k),
            (f"torch foreach SGD n={n}", topt.step, 44 * n),
            (f"fill + torch foreach n={n}", torch_route, 48 * n + 12 * k),
        ):
            dev_us, _wall = time_both(fn, iters)
            rows.append((name, dev_us / 1000, nbytes / GB / (dev_us / 1e6)))
        del topt, params, p, buf, dense
    return rows


def print_rows(rows):
    print(f"{'op':36s} {'ms':>9s} {'GB/s':>8s}")
    for name, ms, bw in rows:
        print(f"{name:36s} {ms:9.4f} {bw:8.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None,
                    help="calls per timed window (default 20; 1000 for the "
                         "microsecond-scale --only wire rows; repeats per "
                         "row, default 15, for --only gauss, topk, "
                         "round2 and reduce)")
    ap.add_argument("--only", default="",
                    choices=["", "colsum", "wire", "gauss", "sparse_step",
                             "topk", "round2", "reduce", "flat_sgd"],
                    help="run just one group of rows")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.only == "sparse_step":
        print_rows(sparse_step_rows(args.iters or 20))
        return
    if args.only == "flat_sgd":
        print_rows(flat_sgd_rows(args.iters or 50))
        return
    if args.only == "colsum":
        print_rows(colsum_rows())
        return
    if args.only == "wire":
        wire_rows(args.iters or 1000)
        return
    if args.only == "gauss":
        gauss_rows(args.iters or 15)
        return
    if args.only == "topk":
        topk_rows(args.iters or 15)
        return
    if args.only == "round2":
        round2_rows(args.iters or 15)
        return
    if args.only == "reduce":
        reduce_rows(args.iters or 15)
        return
    args.iters = args.iters or 20
    g = torch.Generator().manual_seed(0)
    t0 = torch.randn(N, generator=g).cuda()
    r0 = torch.randn(N, generator=g).cuda()
    t = t0.clone()
    r = r0.clone()
    dest = torch.zeros(N, device="cuda")
    m = torch.zeros(N, device="cuda")
    v = torch.zeros(N, device="cuda")
    tau = 0.003  # ~0.1% density on N(0,1) needs tau~3.29; use sel-heavy too
    tau_01pct = 3.2905
    idx, val = H.compact_gt(t, tau_01pct)
    print(f"# N={N}  selected@0.1%={idx.numel()}")

    rows = []

    def bench(name, fn, nbytes):
        # reset inputs: in-place ops (ef_restore) must not poison later rows
        # (an earlier version measured compact at 100% density because
        # ef_restore had blown t up to inf — §5.4 rule 25 of the HIP guide:
        # check the DATA FILL your bench actually runs on)
        t.copy_(t0)
        r.copy_(r0)
        ms = timeit(fn, args.iters) * 1000
        rows.append((name, ms, nbytes / GB / (ms / 1000)))

    bench("ef_restore (t+=r;r=t)", lambda: H.ef_restore_snapshot_(t, r), 4 * 4 * N)
    bench("count_gt", lambda: H.count_gt(t, tau_01pct), 4 * N)
    bench("count_multi_gt x6", lambda: H.count_multi_gt(t, [tau_01pct * 1.03 ** i for i in range(6)]), 4 * N)
    bench("compact_gt @0.1%", lambda: H.compact_gt(t, tau_01pct), 2 * 4 * N)
    bench("kth_abs_value (3-level)", lambda: H.kth_abs_value(t, N // 1000), 3 * 4 * N)
    bench("scatter_add 110k", lambda: H.scatter_add_(dest, idx, val), 3 * 8 * idx.numel())
    bench("fill_sparse_scaled", lambda: H.fill_sparse_scaled_(dest, idx, val, 0.5), 4 * N)
    bench("adam (flat)", lambda: H.fused_adam_(dest, t, m, v, 1e-3, 0.9, 0.999, 1e-6, 0.01), 7 * 4 * N)
    bench("l2norm", lambda: H.l2norm(t), 4 * N)
    # fused EF+count rows: EF is in-place (t,r grow every call), so the
    # timed fn must RESET inputs per iteration or the selection density
    # explodes (rule 25 — this microbench already hit that once, r01-c).
    # Measure (reset + op) and subtract the separately-measured reset.
    gbf = torch.randn(N, generator=g).bfloat16().cuda()
    taus6 = [tau_01pct * 1.03 ** i for i in range(6)]
    reset_ms = timeit(lambda: (t.copy_(t0), r.copy_(r0)), args.iters) * 1000

    def bench_inplace(name, fn, nbytes):
        ms = timeit(lambda: (t.copy_(t0), r.copy_(r0), fn()),
                    args.iters) * 1000 - reset_ms
        rows.append((name, ms, nbytes / GB / (ms / 1000)))

    bench_inplace("ef_count fused (fp32)",
                  lambda: H.compact_adaptive_ef(t, r, None, taus6, N),
                  (4 * 4 + 4) * N)  # EF (r/w t,r) + write-pass read
    bench_inplace("ef_count fused (bf16 g)",
                  lambda: H.compact_adaptive_ef(t, r, gbf, taus6, N),
                  (2 + 4 * 3 + 4) * N)
    bench("zero_at 110k", lambda: H.zero_at_(r, idx), 4 * idx.numel())
    # round-2 kernels
    gsc = H.grad_clip_scale(t, 1.0)
    bench("grad_clip_scale (sumsq+scale)", lambda: H.grad_clip_scale(t, 1.0), 4 * N)
    bench("adam + device clip", lambda: H.fused_adam_(dest, t, m, v, 1e-3, 0.9,
                                                      0.999, 1e-6, 0.01, gsc),
          7 * 4 * N)
    acc64 = torch.zeros(1, dtype=torch.float64, device="cuda")
    bench("sumsq_into", lambda: H.sumsq_into_(acc64, t), 4 * N)
    bench("scatter_gt_credit 110k",
          lambda: H.scatter_gt_credit_(dest, r, idx, val, 0.0, 1.0),
          3 * 8 * idx.numel())

    rows.extend(colsum_rows())
    print_rows(rows)


if __name__ == "__main__":
    main()
