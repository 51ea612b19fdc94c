#!/usr/bin/env python
"""A beam-search step on a forked decode: the attention part of ONE generation step over all layers for B beams, with the worst-case
reorder behind it.

  beam        ForkedCache.update_attend x L, then ForkedCache.reorder with ONE parent for all beams (B - 1 tail copies of TAIL_ROWS
              rows each: kvz_fork_branch_copy, one launch for all layers)
  forked      the forked step alone (what generate_batch pays per step; the parent commit's profiles/fork_decode_ab.txt at the same B)
  sequential  EvictCache.update_attend - B consecutive single-query steps (how B beams decode without the fork)

All in one process on one pruned cache (Qwen2.5-7B geometry, N = 131 072, ratio 0.3, built like tools/fork_decode_bench.py builds its
cache), alternating rounds, hipEvent-timed, every shape warmed first; the copy launch is also timed alone.  Prints ONE JSON line: per B
the median ms per step of the three ways, the copy's share of the beam step, the copy launch alone with its achieved TB/s (bytes read
plus bytes written), and the spread of the rounds (max - min over the median).  Needs a GPU: there is no fallback.

    python tools/beam_decode_bench.py [--rounds 5] [--iters 10] [--ctx 131072]
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

GEOMETRY = ("qwen2.5-7b", 28, 28, 4, 128)   # name, layers, query heads, KV heads, head dim
BEAMS = (2, 4, 8)
TAIL_ROWS = 64      # generated rows every beam's tail holds when a timed step starts


def measure(kv, L, H, Hkv, D, B, rounds, iters, dev):
    from kvzip_amd import ops
    g = torch.Generator(device=dev).manual_seed(B)
    q = torch.randn(L, B, H, 1, D, generator=g, device=dev).half()
    k = torch.randn(L, B, Hkv, 1, D, generator=g, device=dev).half()
    v = torch.randn(L, B, Hkv, 1, D, generator=g, device=dev).half()
    fork = kv.fork(B, tail_capacity=TAIL_ROWS + 2 * (iters + 2) * (rounds + 2))
    seen = kv._seen_tokens
    parents = [0] * B                      # worst case: one beam survives, B - 1 tails are overwritten

    def fork_step():
        for l in range(L):
            fork.update_attend(q[l], k[l], v[l], l)

    def beam_step():
        fork_step()
        fork.reorder(parents)

    def seq_step():   # the B tokens one beam after the other, every beam over all layers
        for b in range(B):
            for l in range(L):
                kv.update_attend(q[l, b:b + 1], k[l, b:b + 1], v[l, b:b + 1], l)

    pairs, rows = [(0, d) for d in range(1, B)], [TAIL_ROWS] * (B - 1)

    def copy_only():
        ops.fork_branch_copy(fork.tail_k, fork.tail_v, pairs, rows)

    def reset():
        fork.tail_len = [[TAIL_ROWS] * B for _ in range(L)]
        fork.active = [True] * B
        kv.slice(seen)

    reset()
    for fn in (fork_step, seq_step, beam_step, fork_step, seq_step, beam_step, copy_only):   # warm (workspaces, tails, code objects)
        fn()
    torch.cuda.synchronize()
    tb, tf, ts, tc = [], [], [], []
    for _ in range(rounds):
        reset()
        tb.append(timed(beam_step, iters))
        reset()
        tf.append(timed(fork_step, iters))
        ts.append(timed(seq_step, iters))
        reset()
        tc.append(timed(copy_only, iters))
    reset()
    mb, mf, ms, mc = (statistics.median(x) for x in (tb, tf, ts, tc))
    spread = lambda x, m: round((max(x) - min(x)) / m, 4)  # noqa: E731
    moved = 2 * 2 * (B - 1) * Hkv * TAIL_ROWS * D * 2 * L    # read + write, K + V, bytes
    return {"B": B, "beam_ms_per_step": round(mb, 4), "fork_ms_per_step": round(mf, 4), "seq_ms_per_step": round(ms, 4),
            "reorder_ms": round(mb - mf, 4), "reorder_share_of_beam_step": round((mb - mf) / mb, 4),
            "reorder_beyond_fork_spread": bool(mb - mf > max(tf) - min(tf)),
            "copy_alone_ms": round(mc, 4), "copy_MB": round(moved / 1e6, 2), "copy_TBps": round(moved / (mc * 1e-3) / 1e12, 4),
            "beam_vs_seq": round(ms / mb, 3), "beam_spread": spread(tb, mb), "fork_spread": spread(tf, mf), "seq_spread": spread(ts, ms),
            "copy_spread": spread(tc, mc), "tail_rows": TAIL_ROWS, "copies": B - 1, "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--ratio", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_decode_bench: needs a GPU (the forked decode has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("beam_decode_bench: at least five rounds of each way")
    dev = "cuda:0"
    name, L, H, Hkv, D = GEOMETRY
    out = {"tool": "beam_decode_bench", "device": torch.cuda.get_device_name(0), "ctx": args.ctx, "ratio": args.ratio, "dtype": "float16",
           "geometry": name, "results": []}
    kv = build_cache(L, H, Hkv, D, args.ctx, args.ratio, dev)
    out["results"] = [measure(kv, L, H, Hkv, D, B, args.rounds, args.iters, dev) for B in BEAMS]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
