#!/usr/bin/env python3
"""Compressor A/B harness: run every compressor mode
on the same model/shape and report ms/step + engine phase breakdown.

Single-process mode exercises the full selection/merge pipeline (comm is
identity); under torchrun it A/Bs the real collectives.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oktopk_amd.comm import init_from_env
from oktopk_amd.config import EngineConfig
from oktopk_amd.trainer import Trainer

COMPRESSORS = ["dense", "oktopk", "topkA", "topkA2", "topkAopt", "topkSA",
               "gtopk", "gaussiank", "gaussiankSA"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert_large")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--density", type=float, default=0.001)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compressors", default=",".join(COMPRESSORS))
    ap.add_argument("--device-exact-topk", action="store_true",
                    help="topkA/topkA2/gtopk select and merge with the exact-k "
                         "HIP ops (EngineConfig.device_exact_topk)")
    ap.add_argument("--device-round2", action="store_true",
                    help="oktopk round-2 tail (global select + residual "
                         "credit) with the HIP op (OkTopkConfig.device_round2)")
    ap.add_argument("--device-reduce", action="store_true",
                    help="oktopk round-1 reduce as the ordered sparse merge "
                         "HIP op (OkTopkConfig.device_reduce)")
    ap.add_argument("--global-recompute-interval", type=int, default=None,
                    help="override OkTopkConfig.global_threshold_recompute_"
                         "interval (1 makes every oktopk step an exact one)")
    args = ap.parse_args()

    comm = init_from_env()
    sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)
    rows = []
    for comp in args.compressors.split(","):
        if comp == "gtopk" and comm.size & (comm.size - 1):
            continue
        cfg = EngineConfig.preset("bert", compressor=comp, density=args.density,
                                  dense_warmup_iters=0,
                                  device_exact_topk=args.device_exact_topk,
                                  device_round2=args.device_round2,
                                  device_reduce=args.device_reduce)
        if args.global_recompute_interval is not None:
            cfg.oktopk.global_threshold_recompute_interval = \
                args.global_recompute_interval
        tr = Trainer(args.model, batch_size=args.batch_size, seq_len=128,
                     comm=comm, cfg=cfg,
                     dtype="bf16" if torch.cuda.is_available() else "fp32")
        for _ in range(args.warmup):
            tr.step()
        tr.capture_graph() and tr.step()
        red = getattr(tr.opt, "reducer", None)
        if red is not None:
            red.timers = {}
        comm.barrier(); sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step()
        sync(); comm.barrier()
        ms = 1000 * (time.perf_counter() - t0) / args.steps
        phases = {}
        if red is not None:
            for _, ph in red.timers.items():
                for k, v in ph.items():
                    phases[k] = phases.get(k, 0.0) + 1000 * v / args.steps
        rows.append((comp, ms, phases))
        del tr
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
    if comm.rank == 0:
        print(f"# {args.model} bs{args.batch_size} density={args.density} "
              f"P={comm.size} steps={args.steps}"
              + (" device_exact_topk" if args.device_exact_topk else "")
              + (" device_round2" if args.device_round2 else "")
              + (" device_reduce" if args.device_reduce else "")
              + (f" global_recompute_interval={args.global_recompute_interval}"
                 if args.global_recompute_interval is not None else ""))
        print(f"{'compressor':12s} {'ms/step':>9s}  phases(ms)")
        for comp, ms, ph in rows:
            pstr = " ".join(f"{k}={v:.2f}" for k, v in sorted(ph.items()))
            print(f"{comp:12s} {ms:9.2f}  {pstr}")


if __name__ == "__main__":
    main()
