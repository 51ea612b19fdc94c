#!/usr/bin/env python
"""Forked decode against sequential decode: the attention part of ONE generation step over all layers for B concurrent queries.

  forked      ForkedCache.update_attend  - one launch per layer serves the B queries and reads the shared rows once
  sequential  EvictCache.update_attend   - B consecutive single-query steps (how the same B tokens are produced without the fork)

Both in one process on one pruned cache (Qwen2.5-7B geometry, N = 131 072, ratio 0.3, built like tools/decode_probe.py builds its
cache; then the Llama-3.1-8B geometry), alternating rounds, hipEvent-timed, every shape warmed first.  Prints ONE JSON line: per
(geometry, B) the median ms per step of both ways, generated tokens per second, the ratio, the spread of the rounds (max - min over
the median) and the fraction of 8 TB/s the forked step reaches on the shared bytes.  Needs a GPU: there is no fallback.

    python tools/fork_decode_bench.py [--rounds 5] [--iters 10] [--ctx 131072]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRIES = [  # name, layers, query heads, KV heads, head dim, branch counts
    ("qwen2.5-7b", 28, 28, 4, 128, (1, 2, 4, 8, 9)),
    ("llama-3.1-8b", 32, 32, 8, 128, (2, 8, 16)),
]
TAIL_ROWS = 32      # rows every branch's tail holds when a timed round starts (a query's worth)


def build_cache(L, H, Hkv, D, N, ratio, dev, sink=32):
    from kvzip_amd.kvcache import EvictCache
    cfg = types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=H, num_key_value_heads=Hkv)
    g = torch.Generator(device=dev).manual_seed(0)
    kv = EvictCache(cfg, (sink, sink + N), device=dev, dtype=torch.float16, verbose=False)
    for l in range(L):
        kv.update(torch.randn(1, Hkv, sink + N, D, generator=g, device=dev).half(),
                  torch.randn(1, Hkv, sink + N, D, generator=g, device=dev).half(), l)
    kv.score = [torch.rand(1, Hkv, N, generator=g, device=dev).half() for _ in range(L)]
    kv.prune(ratio)
    return kv


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(kv, L, H, Hkv, D, B, rounds, iters, dev):
    g = torch.Generator(device=dev).manual_seed(B)
    q = torch.randn(L, B, H, 1, D, generator=g, device=dev).half()
    k = torch.randn(L, B, Hkv, 1, D, generator=g, device=dev).half()
    v = torch.randn(L, B, Hkv, 1, D, generator=g, device=dev).half()
    fork = kv.fork(B, tail_capacity=TAIL_ROWS + 2 * (iters + 2) * (rounds + 2))
    seen = kv._seen_tokens

    def fork_step():
        for l in range(L):
            fork.update_attend(q[l], k[l], v[l], l)

    def seq_step():   # the B tokens one query after the other, every query over all layers
        for b in range(B):
            for l in range(L):
                kv.update_attend(q[l, b:b + 1], k[l, b:b + 1], v[l, b:b + 1], l)

    def reset():
        fork.tail_len = [[TAIL_ROWS] * B for _ in range(L)]
        kv.slice(seen)

    reset()
    fork_step(); seq_step(); fork_step(); seq_step()   # warm both shapes (workspaces, tails, code objects)
    torch.cuda.synchronize()
    tf, ts = [], []
    for _ in range(rounds):
        reset()
        tf.append(timed(fork_step, iters))
        ts.append(timed(seq_step, iters))
    reset()
    mf, ms = statistics.median(tf), statistics.median(ts)
    shared = sum(kv.info["rows_used"]) * D * 2 * 2      # K and V rows of all layers, bytes
    return {"B": B, "fork_ms_per_step": round(mf, 4), "seq_ms_per_step": round(ms, 4),
            "fork_tokens_per_s": round(B / mf * 1e3, 1), "seq_tokens_per_s": round(B / ms * 1e3, 1),
            "ratio": round(ms / mf, 3), "fork_spread": round((max(tf) - min(tf)) / mf, 4), "seq_spread": round((max(ts) - min(ts)) / ms, 4),
            "fork_ms_per_token": round(mf / B, 4), "shared_MB": round(shared / 1e6, 1),
            "fork_fraction_of_8TBps": round(shared / (mf * 1e-3) / 8e12, 3), "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--ratio", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fork_decode_bench: needs a GPU (the forked decode has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("fork_decode_bench: at least five rounds of each way")
    dev = "cuda:0"
    out = {"tool": "fork_decode_bench", "device": torch.cuda.get_device_name(0), "ctx": args.ctx, "ratio": args.ratio, "dtype": "float16",
           "geometries": {}}
    for name, L, H, Hkv, D, Bs in GEOMETRIES:
        kv = build_cache(L, H, Hkv, D, args.ctx, args.ratio, dev)
        out["geometries"][name] = [measure(kv, L, H, Hkv, D, B, args.rounds, args.iters, dev) for B in Bs]
        del kv
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
