#!/usr/bin/env python3
"""Flagship benchmark: BERT-base seq=128, bs=8/GPU, Ok-Topk density=0.1%,
bf16 autocast, synthetic data — the BASELINE.json headline config.  A plain
run sets up, warms up, times the K steps and prints; `--full` adds the in-run
dense-allreduce baseline for the speedup-vs-dense figure.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`, launched
under torch.distributed.run for N>1 (one rank per GPU over RCCL).  Rank 0
prints ONE JSON line.  `--dump-outputs DIR` also writes the last timed step's
loss, parameters and gradients as DIR/<name>.npy (seeded inputs: two runs
with the same arguments start identically).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--model", type=str, default="bert_base")
    p.add_argument("--batch-size", type=int, default=8)
    p.add_argument("--seq-len", type=int, default=128)
    p.add_argument("--density", type=float, default=0.001)
    p.add_argument("--compressor", type=str, default="oktopk")
    p.add_argument("--wire-dtype", type=str, default="bf16", choices=["bf16", "fp32"],
                   help="dtype of sparse values on the wire (indices stay int32)")
    p.add_argument("--balanced-allgather", action="store_true",
                   help="round-2 load-balanced redistribution (equal AllGather blocks)")
    p.add_argument("--pipeline-chunks", type=int, default=1,
                   help="chunked engine pipeline (overlap comm with compress)")
    p.add_argument("--full", action="store_true",
                   help="also run the in-run dense-allreduce baseline arm "
                        "(dense_ms_per_step / speedup_vs_dense); a plain run "
                        "times the headline steps only")
    p.add_argument("--dense-baseline-steps", type=int, default=-1,
                   help="with --full: steps for the in-run dense baseline "
                        "(-1: equal to --steps so the speedup figure compares "
                        "like with like; 0: skip)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps write what the last timed step "
                        "left its caller (loss, model parameters, gradients) "
                        "as DIR/<name>.npy, float32")
    return p.parse_args()


# per dumped array: 4 Mi float32 = 16 MiB, so a dump stays well under 64 MB
DUMP_MAX_ELEMS = 4 * 1024 * 1024


def _sample_flat(tensors):
    """Concatenate `tensors` flat and return them as a float32 numpy array;
    above DUMP_MAX_ELEMS elements, a fixed seeded sample (sorted positions,
    the same for every run with the same shapes)."""
    flat = torch.cat([t.detach().reshape(-1) for t in tensors])
    if flat.numel() > DUMP_MAX_ELEMS:
        g = torch.Generator().manual_seed(20240229)
        idx = torch.randint(0, flat.numel(), (DUMP_MAX_ELEMS,), generator=g)
        flat = flat[idx.sort().values.to(flat.device)]
    return flat.float().cpu().numpy()


def dump_outputs(trainer, outdir):
    """What a caller of trainer.step() holds after the last timed step: the
    returned loss, the updated model parameters and the gradients left on
    them, in model.parameters() order."""
    import numpy as np

    os.makedirs(outdir, exist_ok=True)
    params = [p for p in trainer.model.parameters() if p.requires_grad]
    grads = [p.grad for p in params if p.grad is not None]
    arrays = {
        "loss": np.asarray([trainer.last_loss], dtype=np.float32),
        "params": _sample_flat([p.data for p in params]),
    }
    if grads:
        arrays["grads"] = _sample_flat(grads)
    for name, arr in arrays.items():
        np.save(os.path.join(outdir, f"{name}.npy"), arr)


def timed_steps(trainer, comm, steps):
    """Barrier + device sync bracketed timing of exactly `steps` steps;
    returns max-over-ranks elapsed seconds."""
    dev_sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)
    comm.barrier()
    dev_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step()
    dev_sync()
    comm.barrier()
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], device=comm.device)
    comm.allreduce_(t, op="max")
    return float(t.cpu().item())


def build_trainer(args, comm, compressor):
    from oktopk_amd.config import EngineConfig
    from oktopk_amd.trainer import Trainer

    preset = "bert" if args.model.startswith("bert") else (
        "lstm" if args.model == "lstman4" else "vgg"
    )
    cfg = EngineConfig.preset(preset, compressor=compressor, density=args.density,
                              wire_dtype=args.wire_dtype, dense_warmup_iters=0,
                              balanced_allgather=args.balanced_allgather,
                              pipeline_chunks=args.pipeline_chunks)
    # LSTM recipes run fp32 (MIOpen fused RNN has no bf16 path — 4x
    # slower under autocast, measured); conv/transformer recipes bf16
    dtype = "bf16" if torch.cuda.is_available() else "fp32"
    if args.model.startswith("lstm"):
        dtype = "fp32"
    return Trainer(
        model_name=args.model,
        batch_size=args.batch_size,
        seq_len=args.seq_len,
        comm=comm,
        cfg=cfg,
        dtype=dtype,
    )


def reducer_phase_ms(trainer, steps):
    red = getattr(trainer.opt, "reducer", None)
    if red is None:
        return {}
    totals = {}
    for name, phases in red.timers.items():
        for ph, secs in phases.items():
            totals[ph] = totals.get(ph, 0.0) + secs
    return {ph: 1000.0 * s / max(steps, 1) for ph, s in totals.items()}


def main():
    args = parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

    from oktopk_amd.comm import init_from_env

    comm = init_from_env()
    if args.gpus > 1 and comm.size == 1:
        # --gpus N>1 without a torchrun rendezvous would multiply the
        # reported aggregate by N with only one process doing work
        sys.exit("bench.py --gpus N>1 must be launched via torch.distributed.run "
                 "(one rank per GPU); refusing to report an unmeasured aggregate")
    n_gpus = comm.size if comm.size > 1 else args.gpus
    rank = comm.rank

    # same arguments -> same initial weights and dropout streams (the
    # synthetic batches carry their own per-rank seed), so two builds can be
    # compared output for output
    torch.manual_seed(0)
    trainer = build_trainer(args, comm, args.compressor)
    for _ in range(max(args.warmup, 1)):
        trainer.step()
    captured = trainer.capture_graph()
    if captured:
        trainer.step()  # one replayed step before timing
    # reset phase timers after warmup so per-step phase ms is steady-state;
    # timing_sync drains the queued fwd+bwd before the engine's timed region
    # so "compress" measures the engine, not backward queue depth
    if getattr(trainer.opt, "reducer", None) is not None:
        trainer.opt.reducer.timers = {}
        # under graph replay the engine runs once per step on the flat grad
        # buffer, so the sync is one-per-step and harmless; with live hooks
        # (capture unavailable) it would serialize per-bucket overlap — skip.
        # OKTOPK_PHASE_SYNC=0 disables it (phase_ms then absorbs queue depth;
        # ms_per_step is bracket-timed either way and always honest).
        trainer.opt.reducer.timing_sync = (
            bool(captured) and os.environ.get("OKTOPK_PHASE_SYNC", "1") != "0"
        )
    elapsed = timed_steps(trainer, comm, args.steps)
    ms_per_step = 1000.0 * elapsed / args.steps
    phases = reducer_phase_ms(trainer, args.steps)
    comm_ms = sum(phases.get(p, 0.0) for p in ("alltoall", "allgather", "allreduce"))
    allreduce_ms = sum(phases.values())  # whole sparse-allreduce pipeline
    if args.dump_outputs and rank == 0:
        # before the --full arm below, which steps this trainer further
        dump_outputs(trainer, args.dump_outputs)

    dense_steps = args.dense_baseline_steps if args.full else 0
    if dense_steps < 0:
        # equal steps: at 8 GPUs RCCL warm-up effects make a short dense
        # arm noisy, and the headline speedup figure deserves a
        # like-for-like comparison (VERDICT r01 weak spot 4)
        dense_steps = args.steps
    dense_ms = None
    speedup = None
    if dense_steps > 0 and args.compressor not in ("dense", "none"):
        # INTERLEAVED re-measurement of both arms in alternating chunks:
        # a sequential dense arm runs on a chip already heated by the
        # sparse arm (DVFS give-back) and reads slow, inflating the
        # speedup figure; alternating chunks equalize thermal conditions.
        # The sparse headline above stays the dedicated full run.
        dense_tr = build_trainer(args, comm, "dense")
        for _ in range(max(min(args.warmup, 3), 1)):
            dense_tr.step()
        dense_tr.capture_graph()
        chunk = max(1, min(10, dense_steps // 3 or 1))
        done_d = done_s = 0
        el_d = el_s = 0.0
        while done_d < dense_steps:
            n = min(chunk, dense_steps - done_d)
            el_d += timed_steps(dense_tr, comm, n)
            el_s += timed_steps(trainer, comm, n)
            done_d += n
            done_s += n
        dense_ms = 1000.0 * el_d / done_d
        sparse_ms_i = 1000.0 * el_s / done_s
        speedup = dense_ms / sparse_ms_i

    if args.model.startswith("bert"):
        work_per_step = n_gpus * args.batch_size * args.seq_len
        unit = "tokens/s"
        metric = (f"tokens/s ({args.model} seq{args.seq_len} bs{args.batch_size}/GPU, "
                  f"Ok-Topk density={args.density}, step time & allreduce ms; speedup vs dense)")
    else:
        work_per_step = n_gpus * args.batch_size
        unit = "samples/s"
        metric = (f"samples/s ({args.model} bs{args.batch_size}/GPU, "
                  f"{args.compressor} density={args.density}, step time & allreduce ms; speedup vs dense)")
    value = work_per_step / (ms_per_step / 1000.0)

    if rank == 0:
        out = {
            "metric": metric,
            "value": round(value, 2),
            "unit": unit,
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("fp32" if args.model.startswith("lstm") or not torch.cuda.is_available()
                      else "bf16"),
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": args.batch_size * n_gpus,
                "seq_len": args.seq_len,
                "parallelism": f"dp{n_gpus}",
                "compressor": args.compressor,
                "density": args.density,
                "wire_dtype": args.wire_dtype,
                "allreduce_ms_per_step": round(allreduce_ms, 3),
                "comm_ms_per_step": round(comm_ms, 3),
                "dense_ms_per_step": round(dense_ms, 3) if dense_ms else None,
                "speedup_vs_dense": round(speedup, 3) if speedup else None,
                "speedup_measurement": ("interleaved chunks (thermal-fair): "
                                        "ratio uses the sparse re-measure "
                                        "alongside dense" if speedup else None),
                "hipgraph_fwd_bwd": bool(captured),
                "phase_ms": {k: round(v, 3) for k, v in phases.items()},
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
