"""Attention fwd+bwd per call at BERT-base head geometry (nh 12, hd 64),
graph-timed, arms alternating: the flash kernels (ragged instantiations at
seq % 128 != 0), the explicit matmul+softmax+dropout+matmul chain and torch
SDPA.  Prints one JSON line per (seq, arm): median and min/max over the
runs, in microseconds per call.

    python tools/attn_bench.py --seqs 64 96 200 256 320 --runs 5 --iters 200
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oktopk_amd.ops.fused_attn import fused_attention  # noqa: E402

P_DROP = 0.1


def _split(qkv, nh):
    b, s, _ = qkv.shape
    return qkv.view(b, s, 3, nh, 64).permute(2, 0, 3, 1, 4).unbind(0)


def flash(qkv, mask, nh):
    return fused_attention(qkv, mask, nh, P_DROP, True)


def chain(qkv, mask, nh):
    q, k, v = _split(qkv, nh)
    sc = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(64) + mask
    ctx = torch.matmul(F.dropout(F.softmax(sc, dim=-1), P_DROP, True), v)
    return ctx.transpose(1, 2).reshape(qkv.shape[0], qkv.shape[1], nh * 64)


def sdpa(qkv, mask, nh):
    q, k, v = _split(qkv, nh)
    ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=P_DROP)
    return ctx.transpose(1, 2).reshape(qkv.shape[0], qkv.shape[1], nh * 64)


ARMS = {"flash": flash, "chain": chain, "sdpa": sdpa}


def capture(fn, qkv, mask, gy, nh):
    def step():
        qkv.grad = None
        fn(qkv, mask, nh).backward(gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="+", default=[64, 96, 200, 256, 320])
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--nh", type=int, default=12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_bench needs a GPU"
    os.environ["OKTOPK_FA_ANY_SEQ"] = "1"
    for s in args.seqs:
        gen = torch.Generator().manual_seed(s)
        qkv = (torch.randn(args.bs, s, 3 * args.nh * 64, generator=gen) * 0.5
               ).bfloat16().cuda().requires_grad_(True)
        gy = torch.randn(args.bs, s, args.nh * 64, generator=gen).bfloat16().cuda()
        mask = torch.zeros(args.bs, 1, 1, s, dtype=torch.bfloat16, device="cuda")
        graphs = {n: capture(fn, qkv, mask, gy, args.nh) for n, fn in ARMS.items()}
        times = {n: [] for n in ARMS}
        for _ in range(args.runs):
            for n, g in graphs.items():  # arms alternate within a run
                for _ in range(10):
                    g.replay()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        for n, t in times.items():
            print(json.dumps({"seq": s, "bs": args.bs, "nh": args.nh, "arm": n,
                              "us_median": round(statistics.median(t), 2),
                              "us_min": round(min(t), 2),
                              "us_max": round(max(t), 2), "runs": len(t)}),
                  flush=True)


if __name__ == "__main__":
    main()
