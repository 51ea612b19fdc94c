#!/usr/bin/env python
"""Packed first step of a forked decode against the per-branch first steps: the attention part of the FIRST steps (the query tokens)
of a wave of B queries, over all layers.

  packed      ForkedCache.select_packed + first_step  - per layer ONE kvz_flash_fwd over the shared segments for all B queries' tokens
                                                        and ONE kvz_fork_prefill_tail (append, causal tail attention, LSE merge)
  per branch  ForkedCache.select_branch + first_step  - per layer and branch kvz_dense_append, two kvz_flash_fwd (shared segments,
                                                        tail) and kvz_attn_merge_lse: B reads of the shared rows

Both in one process on forks of one pruned cache (Qwen2.5-7B geometry, N = 131 072, ratio 0.3, built like tools/fork_decode_bench.py
builds its cache; one line of the Llama-3.1-8B geometry), on the same inputs, alternating rounds, hipEvent-timed, every shape warmed
first.  Prints a table and then ONE JSON line: per (geometry, B, tokens per query) the median ms per wave of both ways, the ratio and
the spread of the rounds (max - min over the median).  Needs a GPU: there is no fallback.  One geometry per process, so that a
caller can give every GPU step a time limit of its own:

    timeout -k 10 600 python tools/fork_prefill_bench.py --geometry qwen2.5-7b   [--rounds 5] [--iters 3] [--ctx 131072]
    timeout -k 10 600 python tools/fork_prefill_bench.py --geometry llama-3.1-8b
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fork_decode_bench import build_cache, timed  # noqa: E402

GEOMETRIES = {  # name: layers, query heads, KV heads, head dim, branch counts, tokens per query
    "qwen2.5-7b": (28, 28, 4, 128, (2, 4, 8, 9), (16, 48, 160)),
    "llama-3.1-8b": (32, 32, 8, 128, (8,), (48,)),
}


def measure(kv, L, H, Hkv, D, B, n, rounds, iters, dev):
    g = torch.Generator(device=dev).manual_seed(B * 1000 + n)
    T = B * n
    # [1, H, T, D] views of [1, T, H, D] storage, as the projections hand them over
    q = [torch.randn(1, T, H, D, generator=g, device=dev).half().transpose(1, 2) for _ in range(L)]
    k = [torch.randn(1, T, Hkv, D, generator=g, device=dev).half().transpose(1, 2) for _ in range(L)]
    v = [torch.randn(1, T, Hkv, D, generator=g, device=dev).half().transpose(1, 2) for _ in range(L)]
    fa, fb = kv.fork(B, tail_capacity=n), kv.fork(B, tail_capacity=n)
    branches, lengths = list(range(B)), [n] * B

    def packed():
        fa.tail_len = [[0] * B for _ in range(L)]
        fa.select_packed(branches, lengths)
        for l in range(L):
            fa.first_step(q[l], k[l], v[l], l)

    def per_branch():
        fb.tail_len = [[0] * B for _ in range(L)]
        for b in range(B):
            fb.select_branch(b)
            sl = slice(b * n, (b + 1) * n)
            for l in range(L):
                fb.first_step(q[l][:, :, sl], k[l][:, :, sl], v[l][:, :, sl], l)

    packed(); per_branch(); packed(); per_branch()      # warm both shapes (tails, workspaces, code objects)
    torch.cuda.synchronize()
    same = all(torch.equal(fa.tail_k[l], fb.tail_k[l]) and torch.equal(fa.tail_v[l], fb.tail_v[l]) for l in range(L))
    tp, tb = [], []
    for _ in range(rounds):
        tp.append(timed(packed, iters))
        tb.append(timed(per_branch, iters))
    mp, mb = statistics.median(tp), statistics.median(tb)
    return {"B": B, "tokens_per_query": n, "packed_ms_per_wave": round(mp, 4), "per_branch_ms_per_wave": round(mb, 4),
            "ratio": round(mb / mp, 3), "packed_spread": round((max(tp) - min(tp)) / mp, 4),
            "per_branch_spread": round((max(tb) - min(tb)) / mb, 4), "tails_identical": bool(same), "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=sorted(GEOMETRIES), default="qwen2.5-7b")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--ratio", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fork_prefill_bench: needs a GPU (the forked decode has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("fork_prefill_bench: at least five rounds of each way")
    dev = "cuda:0"
    L, H, Hkv, D, Bs, ns = GEOMETRIES[args.geometry]
    kv = build_cache(L, H, Hkv, D, args.ctx, args.ratio, dev)
    rows = [measure(kv, L, H, Hkv, D, B, n, args.rounds, args.iters, dev) for n in ns for B in Bs]
    print(f"{args.geometry}  ctx {args.ctx}  ratio {args.ratio}  fp16  (ms per wave: attention of the first steps, {L} layers)")
    print(f"{'B':>3} {'tokens':>6} {'packed':>10} {'per branch':>11} {'ratio':>7} {'spread p':>9} {'spread b':>9}")
    for r in rows:
        print(f"{r['B']:>3} {r['tokens_per_query']:>6} {r['packed_ms_per_wave']:>10.3f} {r['per_branch_ms_per_wave']:>11.3f} "
              f"{r['ratio']:>7.2f} {r['packed_spread']:>9.3f} {r['per_branch_spread']:>9.3f}")
    print(json.dumps({"tool": "fork_prefill_bench", "device": torch.cuda.get_device_name(0), "geometry": args.geometry, "ctx": args.ctx,
                      "ratio": args.ratio, "dtype": "float16", "rows": rows}))


if __name__ == "__main__":
    main()
