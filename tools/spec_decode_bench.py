#!/usr/bin/env python
"""The verify step of speculative decoding against the existing ways to run the same forward: the attention part of ONE step of t
consecutive positions over all layers, on one pruned cache.

  (a) verify      EvictCache.verify_attend              - kvz_spec_attn_append: two launches per layer, the kept rows read once
                                                           (twice beyond 32 query rows per KV head)
  (b) existing    EvictCache.update + prepare + attend  - what a forward of t tokens on a pruned cache ran before: kvz_append_inplace
                                                           and kvz_varlen_attn with q_len = t
  (c) sequential  t x EvictCache.update_attend          - the t tokens as t decode steps

All three in one process on one cache (Qwen2.5-7B geometry, N = 131 072, ratio 0.3, fp16, built like tools/fork_decode_bench.py builds
its cache; then the Llama-3.1-8B geometry), alternating rounds, hipEvent-timed, every shape warmed first.  Prints a table and writes it
(with one JSON line) to --out: per (geometry, t) the median ms per step of the three ways, the round-to-round spread (max - min) /
median, the fraction of 8 TB/s the verify step reaches on the kept bytes, the break-even acceptance (a at t) / (a at t = 1) in tokens
per step, and `slower_beyond_spread` where (a) loses to (b) by more than the larger of the two spreads.  Needs a GPU: no fallback.

    python tools/spec_decode_bench.py [--rounds 5] [--iters 10] [--ctx 131072] [--out profiles/spec_decode_ab.txt]
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

GEOMETRIES = [  # name, layers, query heads, KV heads, head dim, positions per step
    ("qwen2.5-7b", 28, 28, 4, 128, (1, 2, 4, 5, 8, 9)),
    ("llama-3.1-8b", 32, 32, 8, 128, (1, 4, 8, 16)),      # (t = 1: the denominator of the break-even acceptance)
]


def measure(kv, L, H, Hkv, D, t, rounds, iters, dev):
    g = torch.Generator(device=dev).manual_seed(t)
    q = torch.randn(L, 1, H, t, D, generator=g, device=dev).half()
    k = torch.randn(L, 1, Hkv, t, D, generator=g, device=dev).half()
    v = torch.randn(L, 1, Hkv, t, D, generator=g, device=dev).half()
    q1 = [q[:, :, :, p:p + 1].contiguous() for p in range(t)]      # the positions one by one, for (c)
    k1 = [k[:, :, :, p:p + 1].contiguous() for p in range(t)]
    v1 = [v[:, :, :, p:p + 1].contiguous() for p in range(t)]
    seen = kv._seen_tokens

    def verify_step():
        for l in range(L):
            kv.verify_attend(q[l], k[l], v[l], l)

    def existing_step():
        for l in range(L):
            kv.update(k[l], v[l], l)
            qq, kk, vv, info = kv.prepare(q[l], kv.key_cache[l], kv.value_cache[l], l)
            kv.attend(qq, kk, vv, info, causal=True)

    def seq_step():
        for p in range(t):
            for l in range(L):
                kv.update_attend(q1[p][l], k1[p][l], v1[p][l], l)

    ways = (("verify", verify_step), ("existing", existing_step), ("sequential", seq_step))
    for _ in range(2):      # warm every shape (workspaces, code objects)
        for _, fn in ways:
            kv.slice(seen)
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in ways}
    for _ in range(rounds):
        for name, fn in ways:
            kv.slice(seen)      # every round starts from the pruned cache: the steps of a round append iters * t rows
            times[name].append(timed(fn, iters))
    kv.slice(seen)
    med = {n: statistics.median(x) for n, x in times.items()}
    spread = {n: (max(x) - min(x)) / med[n] for n, x in times.items()}
    kept = sum(kv.info["rows_used"]) * D * 2 * 2      # K and V rows of all layers, bytes
    return {"t": t, "rows_per_kv_head": t * (H // Hkv), "verify_ms": round(med["verify"], 4), "existing_ms": round(med["existing"], 4),
            "sequential_ms": round(med["sequential"], 4), "verify_spread": round(spread["verify"], 4),
            "existing_spread": round(spread["existing"], 4), "sequential_spread": round(spread["sequential"], 4),
            "kept_MB": round(kept / 1e6, 1), "verify_fraction_of_8TBps": round(kept / (med["verify"] * 1e-3) / 8e12, 3),
            "slower_beyond_spread": bool(med["verify"] > med["existing"] * (1 + max(spread["verify"], spread["existing"]))),
            "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--ratio", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_decode_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spec_decode_bench: needs a GPU (the verify step has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("spec_decode_bench: at least five rounds of each way")
    dev = "cuda:0"
    res = {"tool": "spec_decode_bench", "device": torch.cuda.get_device_name(0), "ctx": args.ctx, "ratio": args.ratio, "dtype": "float16",
           "geometries": {}}
    lines = [f"spec_decode_bench: attention part of one verify step over all layers, N = {args.ctx}, ratio {args.ratio}, fp16, "
             f"{args.rounds} alternating rounds x {args.iters} steps, {res['device']}",
             "(a) verify = verify_attend, (b) existing = update + prepare + attend with q_len = t, (c) sequential = t x update_attend",
             "spread = (max - min) / median over the rounds; break-even = (a at t) / (a at t = 1) tokens per step", ""]
    for name, L, H, Hkv, D, ts in GEOMETRIES:
        kv = build_cache(L, H, Hkv, D, args.ctx, args.ratio, dev)
        # (the slack holds the rows of one round of every way)
        if kv.slack < max(ts) * (args.iters + 2):
            kv._grow_slack(max(ts) * (args.iters + 2))
        rows = [measure(kv, L, H, Hkv, D, t, args.rounds, args.iters, dev) for t in ts]
        base = rows[0]["verify_ms"]
        for r in rows:
            r["break_even_tokens_per_step"] = round(r["verify_ms"] / base, 3)
        res["geometries"][name] = rows
        lines.append(f"{name} (L {L}, H {H}, Hkv {Hkv}, D {D}; kept rows {rows[0]['kept_MB']} MB)")
        lines.append(f"{'t':>3} {'rows':>4} | {'(a) ms':>8} {'spread':>7} | {'(b) ms':>8} {'spread':>7} | {'(c) ms':>8} {'spread':>7} | "
                     f"{'of 8TB/s':>8} {'break-even':>10}  flag")
        for r in rows:
            lines.append(f"{r['t']:>3} {r['rows_per_kv_head']:>4} | {r['verify_ms']:>8.4f} {r['verify_spread']:>7.1%} | "
                         f"{r['existing_ms']:>8.4f} {r['existing_spread']:>7.1%} | {r['sequential_ms']:>8.4f} {r['sequential_spread']:>7.1%} | "
                         f"{r['verify_fraction_of_8TBps']:>8.3f} {r['break_even_tokens_per_step']:>10.3f}  "
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
