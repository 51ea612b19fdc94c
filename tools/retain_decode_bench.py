#!/usr/bin/env python
"""Decode on the non-evicting cache: the attention part of ONE generation step over all layers, through the index of kept positions
against the gather route it replaces, and against the evicting cache under the same mask.

  (a) indexed   RetainCache.update_attend               - kvz_retain_attn_append: the kept rows read where they lie in the dense store
  (b) gather    RetainCache.update + prepare + attend   - per layer: plan, one host round trip, gather of every kept K, V row into a
                                                           flat copy, kvz_varlen_attn on the copy (the same cache, indexed or not)
  (c) evict     EvictCache.update_attend                - kvz_varlen_attn_append on the compacted cache under the same mask

All three in one process (Qwen2.5-7B geometry, N = 131 072, fp16; ONE dense K, V that the evicting cache compacts from), per ratio
0.1 / 0.3 / 0.6 / 1.0 in alternating rounds, hipEvent-timed, every shape warmed first.  Prints a table and writes it (with one JSON
line) to --out: per ratio the median ms per step of the three arms, the round-to-round spread (max - min) / median, the fraction of
8 TB/s arm (a) reaches on the kept bytes, (a) / (c) - the price of rows that are scattered instead of consecutive, reported and not
gated - and `slower_beyond_spread` where (a) is slower than (b) by more than the larger of the two spreads: such a shape becomes a rule
in RetainCache.index_takes that sends it down the gather route.  Needs a GPU: no fallback.

    python tools/retain_decode_bench.py [--rounds 5] [--iters 10] [--ctx 131072] [--out profiles/retain_decode_ab.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fork_decode_bench import timed  # noqa: E402

GEOMETRY = ("qwen2.5-7b", 28, 28, 4, 128)      # name, layers, query heads, KV heads, head dim
RATIOS = (0.1, 0.3, 0.6, 1.0)


def build_retain(L, H, Hkv, D, N, dev, sink=32):
    from kvzip_amd.kvcache import RetainCache
    cfg = types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=H, num_key_value_heads=Hkv)
    g = torch.Generator(device=dev).manual_seed(0)
    kr = RetainCache(cfg, (sink, sink + N), device=dev, dtype=torch.float16, verbose=False)
    for l in range(L):
        kr.update(torch.randn(1, Hkv, sink + N, D, generator=g, device=dev).half(),
                  torch.randn(1, Hkv, sink + N, D, generator=g, device=dev).half(), l)
    kr.score = [torch.rand(1, Hkv, N, generator=g, device=dev).half() for _ in range(L)]
    return kr, cfg


def evict_from(kr, cfg, ratio, dev):
    """An EvictCache over the SAME dense rows and scores, pruned at `ratio` (it compacts into buffers of its own and lets go of the
    dense store, which stays the retaining cache's)."""
    from kvzip_amd.kvcache import EvictCache
    ke = EvictCache(cfg, (kr.start_idx, kr.end_idx), device=dev, dtype=torch.float16, verbose=False)
    ke.adopt_dense(kr._store_k, kr._store_v, kr._fill[0])
    ke.score = kr.score
    ke.prune(ratio)
    return ke


def measure(kr, ke, L, H, Hkv, D, ratio, rounds, iters, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    q = torch.randn(L, 1, H, 1, D, generator=g, device=dev).half()
    k = torch.randn(L, 1, Hkv, 1, D, generator=g, device=dev).half()
    v = torch.randn(L, 1, Hkv, 1, D, generator=g, device=dev).half()
    seen_r, seen_e = kr._seen_tokens, ke._seen_tokens
    assert kr.index_takes(q[0]), "the indexed route does not take this shape"

    def indexed_step():
        for l in range(L):
            kr.update_attend(q[l], k[l], v[l], l)

    def gather_step():
        for l in range(L):
            kr.update(k[l], v[l], l)
            qq, kk, vv, info = kr.prepare(q[l], kr.key_cache[l], kr.value_cache[l], l)
            kr.attend(qq, kk, vv, info, causal=True)

    def evict_step():
        for l in range(L):
            ke.update_attend(q[l], k[l], v[l], l)

    def reset():
        kr.slice(seen_r)
        ke.slice(seen_e)

    ways = (("indexed", indexed_step), ("gather", gather_step), ("evict", evict_step))
    for _ in range(2):      # warm every shape (workspaces, code objects)
        for _, fn in ways:
            reset()
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ways}
    for _ in range(rounds):
        for name, fn in ways:
            reset()      # every round starts from the pruned cache: the steps of a round append iters rows
            times[name].append(timed(fn, iters))
    reset()
    med = {n: statistics.median(x) for n, x in times.items()}
    spread = {n: (max(x) - min(x)) / med[n] for n, x in times.items()}
    kept = kr._index.total * D * 2 * 2      # K and V rows of all layers, bytes
    return {"ratio": ratio, "indexed_ms": round(med["indexed"], 4), "gather_ms": round(med["gather"], 4), "evict_ms": round(med["evict"], 4),
            "indexed_spread": round(spread["indexed"], 4), "gather_spread": round(spread["gather"], 4),
            "evict_spread": round(spread["evict"], 4), "kept_MB": round(kept / 1e6, 1), "index_MB": round(kr._index.total * 4 / 1e6, 1),
            "indexed_fraction_of_8TBps": round(kept / (med["indexed"] * 1e-3) / 8e12, 3),
            "indexed_over_evict": round(med["indexed"] / med["evict"], 3), "gather_over_indexed": round(med["gather"] / med["indexed"], 3),
            "slower_beyond_spread": bool(med["indexed"] > med["gather"] * (1 + max(spread["indexed"], spread["gather"]))),
            "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retain_decode_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retain_decode_bench: needs a GPU (the indexed attention has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("retain_decode_bench: at least five rounds of each arm")
    dev = "cuda:0"
    name, L, H, Hkv, D = GEOMETRY
    res = {"tool": "retain_decode_bench", "device": torch.cuda.get_device_name(0), "ctx": args.ctx, "dtype": "float16", "geometry": name,
           "rows": []}
    lines = [f"retain_decode_bench: attention part of one decode step over all layers, {name} (L {L}, H {H}, Hkv {Hkv}, D {D}), "
             f"N = {args.ctx}, fp16, {args.rounds} alternating rounds x {args.iters} steps, {res['device']}",
             "(a) indexed = RetainCache.update_attend, (b) gather = update + prepare + attend on the same cache, "
             "(c) evict = EvictCache.update_attend under the same mask",
             "spread = (max - min) / median over the rounds; (a)/(c) = the price of scattered rows (reported, not gated)", "",
             f"{'ratio':>5} {'kept MB':>8} | {'(a) ms':>8} {'spread':>7} | {'(b) ms':>8} {'spread':>7} | {'(c) ms':>8} {'spread':>7} | "
             f"{'of 8TB/s':>8} {'(b)/(a)':>8} {'(a)/(c)':>8}  flag"]
    kr, cfg = build_retain(L, H, Hkv, D, args.ctx, dev)
    for ratio in RATIOS:
        kr.prune(ratio)
        ke = evict_from(kr, cfg, ratio, dev)
        r = measure(kr, ke, L, H, Hkv, D, ratio, args.rounds, args.iters, dev)
        res["rows"].append(r)
        print(f"ratio {ratio}: measured", file=sys.stderr, flush=True)
        lines.append(f"{r['ratio']:>5} {r['kept_MB']:>8.1f} | {r['indexed_ms']:>8.4f} {r['indexed_spread']:>7.1%} | {r['gather_ms']:>8.4f} "
                     f"{r['gather_spread']:>7.1%} | {r['evict_ms']:>8.4f} {r['evict_spread']:>7.1%} | {r['indexed_fraction_of_8TBps']:>8.3f} "
                     f"{r['gather_over_indexed']:>8.3f} {r['indexed_over_evict']:>8.3f}  "
                     f"{'slower_beyond_spread' if r['slower_beyond_spread'] else ''}")
        del ke
        torch.cuda.empty_cache()
    lines += ["", json.dumps(res)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
