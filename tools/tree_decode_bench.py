#!/usr/bin/env python
"""The tree verify step of speculative decoding against the chain verify step: the attention part of ONE step of t new positions
over all layers, on one pruned cache.

  (a) tree        EvictCache.verify_attend inside verifying(tree=...)  - kvz_tree_attn_append with a seeded random tree of t nodes
  (b) chain       EvictCache.verify_attend                              - kvz_spec_attn_append with the same t: the yardstick of (a)
  (c) tree+keep   (a), then EvictCache.keep_path in its worst case      - the path 1, 2, .., t - 1: every kept row moves, in every layer
  (d) sequential  t x EvictCache.update_attend                          - the t tokens as t decode steps

All four in one process on one cache (Qwen2.5-7B geometry, N = 131 072, ratio 0.3, fp16, built like tools/fork_decode_bench.py builds
its cache; then the Llama-3.1-8B geometry), alternating rounds, hipEvent-timed, every shape warmed first, every timed call under a
wall-clock limit (--limit seconds: the tool ends instead of waiting on a step that does not come back).  The shared items of (a) and
(b) are the same code, so (a) is expected to equal (b); a shape where (a) exceeds (b) by more than the larger of the two round-to-round
spreads is flagged `slower_beyond_spread`.  Prints a table and writes it (with one JSON line) to --out: per (geometry, t) the median
ms per step of the four ways, the spread (max - min) / median, and the share of keep_path in a step of (c).  What it does NOT measure:
how many more tokens a tree gets accepted than a chain on real answers, and end-to-end tokens per second - this repository holds no
real model.  Needs a GPU: no fallback.

    python tools/tree_decode_bench.py [--rounds 5] [--iters 10] [--ctx 131072] [--out profiles/tree_decode_ab.txt]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fork_decode_bench import build_cache  # noqa: E402

GEOMETRIES = [  # name, layers, query heads, KV heads, head dim, nodes per step
    ("qwen2.5-7b", 28, 28, 4, 128, (2, 4, 5, 9)),
    ("llama-3.1-8b", 32, 32, 8, 128, (4, 8, 16)),
]


def _limited(fn, iters, limit):
    """ms per call of fn over iters calls (hipEvents, as fork_decode_bench.timed), ending the tool when they are not done in time."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    deadline = time.monotonic() + limit
    while not b.query():
        if time.monotonic() > deadline:
            sys.exit(f"tree_decode_bench: {iters} steps did not come back within {limit} s")
        time.sleep(0.0002)
    return a.elapsed_time(b) / iters


def measure(kv, L, H, Hkv, D, t, rounds, iters, limit, dev):
    g = torch.Generator(device=dev).manual_seed(t)
    q = torch.randn(L, 1, H, t, D, generator=g, device=dev).half()
    k = torch.randn(L, 1, Hkv, t, D, generator=g, device=dev).half()
    v = torch.randn(L, 1, Hkv, t, D, generator=g, device=dev).half()
    q1 = [q[:, :, :, p:p + 1].contiguous() for p in range(t)]      # the positions one by one, for (d)
    k1 = [k[:, :, :, p:p + 1].contiguous() for p in range(t)]
    v1 = [v[:, :, :, p:p + 1].contiguous() for p in range(t)]
    rng = random.Random(t)
    parents = [-1] + [rng.randrange(i) for i in range(1, t)]
    shifted = list(range(1, t))                                     # every kept row moves
    seen = kv._seen_tokens

    def chain_step():
        for l in range(L):
            kv.verify_attend(q[l], k[l], v[l], l)

    def tree_step():
        with kv.verifying(tree=parents):
            for l in range(L):
                kv.verify_attend(q[l], k[l], v[l], l)

    def tree_keep_step():
        tree_step()
        kv.keep_path(shifted, t)

    def seq_step():
        for p in range(t):
            for l in range(L):
                kv.update_attend(q1[p][l], k1[p][l], v1[p][l], l)

    ways = (("tree", tree_step), ("chain", chain_step), ("tree_keep", tree_keep_step), ("sequential", seq_step))
    for _ in range(2):      # warm every shape (workspaces, code objects)
        for _, fn in ways:
            kv.slice(seen)
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ways}
    for _ in range(rounds):
        for name, fn in ways:
            kv.slice(seen)      # every round starts from the pruned cache: the steps of a round append up to iters * t rows
            times[name].append(_limited(fn, iters, limit))
    kv.slice(seen)
    med = {n: statistics.median(x) for n, x in times.items()}
    spread = {n: (max(x) - min(x)) / med[n] for n, x in times.items()}
    return {"t": t, "rows_per_kv_head": t * (H // Hkv), "parents": parents,
            "tree_ms": round(med["tree"], 4), "chain_ms": round(med["chain"], 4), "tree_keep_ms": round(med["tree_keep"], 4),
            "sequential_ms": round(med["sequential"], 4), "tree_spread": round(spread["tree"], 4), "chain_spread": round(spread["chain"], 4),
            "tree_keep_spread": round(spread["tree_keep"], 4), "sequential_spread": round(spread["sequential"], 4),
            "tree_over_chain": round(med["tree"] / med["chain"], 4),
            "keep_path_share": round(max(0.0, med["tree_keep"] - med["tree"]) / med["tree_keep"], 4),
            "slower_beyond_spread": bool(med["tree"] > med["chain"] * (1 + max(spread["tree"], spread["chain"]))),
            "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--ratio", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=60, help="wall-clock seconds one timed call may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_decode_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tree_decode_bench: needs a GPU (the verify step has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("tree_decode_bench: at least five rounds of each way")
    dev = "cuda:0"
    res = {"tool": "tree_decode_bench", "device": torch.cuda.get_device_name(0), "ctx": args.ctx, "ratio": args.ratio, "dtype": "float16",
           "geometries": {}}
    lines = [f"tree_decode_bench: attention part of one verify step over all layers, N = {args.ctx}, ratio {args.ratio}, fp16, "
             f"{args.rounds} alternating rounds x {args.iters} steps, {res['device']}",
             "(a) tree = verify_attend in verifying(tree=seeded random tree), (b) chain = verify_attend, (c) = (a) + keep_path(1 .. t-1),",
             "(d) sequential = t x update_attend; spread = (max - min) / median over the rounds; keep = ((c) - (a)) / (c)",
             "not measured: the acceptance gain of a tree over a chain on real answers, end-to-end tokens per second", ""]
    for name, L, H, Hkv, D, ts in GEOMETRIES:
        kv = build_cache(L, H, Hkv, D, args.ctx, args.ratio, dev)
        # (the slack holds the rows of one round of every way)
        if kv.slack < max(ts) * (args.iters + 2):
            kv._grow_slack(max(ts) * (args.iters + 2))
        rows = [measure(kv, L, H, Hkv, D, t, args.rounds, args.iters, args.limit, dev) for t in ts]
        res["geometries"][name] = rows
        lines.append(f"{name} (L {L}, H {H}, Hkv {Hkv}, D {D})")
        lines.append(f"{'t':>3} {'rows':>4} | {'(a) ms':>8} {'spread':>7} | {'(b) ms':>8} {'spread':>7} | {'(a)/(b)':>7} | {'(c) ms':>8} {'spread':>7} "
                     f"{'keep':>6} | {'(d) ms':>8} {'spread':>7}  flag")
        for r in rows:
            lines.append(f"{r['t']:>3} {r['rows_per_kv_head']:>4} | {r['tree_ms']:>8.4f} {r['tree_spread']:>7.1%} | {r['chain_ms']:>8.4f} "
                         f"{r['chain_spread']:>7.1%} | {r['tree_over_chain']:>7.3f} | {r['tree_keep_ms']:>8.4f} {r['tree_keep_spread']:>7.1%} "
                         f"{r['keep_path_share']:>6.1%} | {r['sequential_ms']:>8.4f} {r['sequential_spread']:>7.1%}  "
                         f"{'slower_beyond_spread' if r['slower_beyond_spread'] else ''}")
        lines.append("")
        del kv
        torch.cuda.empty_cache()
    lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
