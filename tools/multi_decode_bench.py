#!/usr/bin/env python
"""Batched decode over several independent caches against sequential decode: the attention part of ONE generation step over all
layers for B users, each with a pruned cache of its own.

  batched     CacheBatch.update_attend   - one launch per layer serves the B caches (work items cut from the sum of all their lengths)
  sequential  EvictCache.update_attend   - B consecutive single-cache steps (how the same B tokens are produced without the batch)

Both in one process on the same caches (Qwen2.5-7B geometry, ratio 0.3, built like tools/fork_decode_bench.py builds its cache),
alternating rounds, hipEvent-timed, every shape warmed first.  Shapes: N in {8 192, 32 768, 131 072} x B in {2, 4, 8}, and one mixed
batch - a 131 072-token cache with three 8 192-token ones.  Prints ONE JSON line: per shape the median ms per step of both ways,
generated tokens per second, the ratio, the spread of the rounds (max - min over the median) and the fraction of 8 TB/s the batched
step reaches on the K,V bytes of the B caches.  Needs a GPU: there is no fallback.

    python tools/multi_decode_bench.py [--rounds 5] [--iters 10] [--ctx 8192 32768 131072] [--batches 2 4 8]
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

L, H, HKV, D = 28, 28, 4, 128      # Qwen2.5-7B


def build_cache(N, ratio, dev, seed, sink=32):
    from kvzip_amd.kvcache import EvictCache
    cfg = types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=H, num_key_value_heads=HKV)
    g = torch.Generator(device=dev).manual_seed(seed)
    kv = EvictCache(cfg, (sink, sink + N), device=dev, dtype=torch.float16, verbose=False)
    for l in range(L):
        kv.update(torch.randn(1, HKV, sink + N, D, generator=g, device=dev).half(),
                  torch.randn(1, HKV, sink + N, D, generator=g, device=dev).half(), l)
    kv.score = [torch.rand(1, HKV, N, generator=g, device=dev).half() for _ in range(L)]
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


def measure(name, kvs, rounds, iters, dev):
    from kvzip_amd.kvcache import CacheBatch
    B = len(kvs)
    g = torch.Generator(device=dev).manual_seed(B)
    q = torch.randn(L, B, H, 1, D, generator=g, device=dev).half()
    k = torch.randn(L, B, HKV, 1, D, generator=g, device=dev).half()
    v = torch.randn(L, B, HKV, 1, D, generator=g, device=dev).half()
    batch = CacheBatch(kvs)
    seen = [kv._seen_tokens for kv in kvs]

    def batch_step():
        for l in range(L):
            batch.update_attend(q[l], k[l], v[l], l)

    def seq_step():   # the B tokens one user after the other, every user over all layers
        for b, kv in enumerate(kvs):
            for l in range(L):
                kv.update_attend(q[l, b:b + 1], k[l, b:b + 1], v[l, b:b + 1], l)

    def reset():
        for kv, s in zip(kvs, seen):
            kv.slice(s)

    batch_step(); seq_step(); batch_step(); seq_step()   # warm both shapes (workspaces, code objects)
    torch.cuda.synchronize()
    tb, ts = [], []
    for _ in range(rounds):
        reset()
        tb.append(timed(batch_step, iters))
        ts.append(timed(seq_step, iters))
    reset()
    mb, ms = statistics.median(tb), statistics.median(ts)
    nbytes = sum(sum(kv.info["rows_used"]) for kv in kvs) * D * 2 * 2      # K and V rows of all layers of all caches
    return {"shape": name, "B": B, "batch_ms_per_step": round(mb, 4), "seq_ms_per_step": round(ms, 4),
            "batch_tokens_per_s": round(B / mb * 1e3, 1), "seq_tokens_per_s": round(B / ms * 1e3, 1), "ratio": round(ms / mb, 3),
            "batch_spread": round((max(tb) - min(tb)) / mb, 4), "seq_spread": round((max(ts) - min(ts)) / ms, 4),
            "slower_beyond_spread": bool(mb - ms > max(max(tb) - min(tb), max(ts) - min(ts))),
            "kv_MB": round(nbytes / 1e6, 1), "batch_fraction_of_8TBps": round(nbytes / (mb * 1e-3) / 8e12, 3),
            "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ctx", type=int, nargs="+", default=[8192, 32768, 131072])
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--ratio", type=float, default=0.3)
    ap.add_argument("--no-mixed", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("multi_decode_bench: needs a GPU (the batched decode has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("multi_decode_bench: at least five rounds of each way")
    dev = "cuda:0"
    out = {"tool": "multi_decode_bench", "device": torch.cuda.get_device_name(0), "geometry": "qwen2.5-7b", "ratio": args.ratio,
           "dtype": "float16", "shapes": []}
    small = None
    for N in args.ctx:
        kvs = [build_cache(N, args.ratio, dev, seed=b) for b in range(max(args.batches))]
        for B in args.batches:
            out["shapes"].append(measure(f"N{N}", kvs[:B], args.rounds, args.iters, dev))
        if N == 8192:
            small = kvs[:3]
        if N == 131072 and small is not None and not args.no_mixed:
            out["shapes"].append(measure("mixed 131072 + 3 x 8192", [kvs[0]] + small, args.rounds, args.iters, dev))
        del kvs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
