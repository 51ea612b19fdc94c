#!/usr/bin/env python
"""Tightening a pruned cache (0.6 -> 0.3) against pruning the dense cache at 0.3, on one device in one process.

  tighten   EvictCache.tighten on a cache pruned at --from-ratio: selection on the retained scores, plan of the new mask + subset
            check, gather from the ragged layout (kvz_recompact_layers) - the three stages hipEvent-timed one by one, and the whole
            call once more on a second cache
  fresh     EvictCache.prepare_init at --ratio from the dense K,V (plan + kvz_compact_layers), selection excluded

Qwen2.5-7B geometry (L 28, Hkv 4, D 128, N = 131 072, fp16, synthetic scores; the dense K,V are built once and adopted by every
cache, so a round costs two prunes at --from-ratio beside the timed work).  Alternating rounds; the gather kernels themselves are read
from the library's own event brackets (kvz_prof_read: "recompact_gather", "compact_gather").  Prints ONE JSON line: medians, the spread
of the rounds (max - min over the median) and the achieved TB/s on the algorithmic bytes (2 x kept rows x row bytes x (K and V) + the
mask reads).  Needs a GPU: there is no fallback.  Run it under a time limit of its own (`timeout -k 10 300 python tools/tighten_bench.py`).

    python tools/tighten_bench.py [--rounds 7] [--ctx 131072] [--from-ratio 0.6] [--ratio 0.3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, H, HKV, D, SINK = 28, 28, 4, 128, 32


class Timer:
    def __init__(self):
        self.ev = [torch.cuda.Event(enable_timing=True)]
        self.ev[0].record()

    def mark(self):
        self.ev.append(torch.cuda.Event(enable_timing=True))
        self.ev[-1].record()

    def ms(self):
        self.ev[-1].synchronize()
        return [a.elapsed_time(b) for a, b in zip(self.ev, self.ev[1:])]


def prof_read(lib, name):
    ms, n = ctypes.c_double(0), ctypes.c_int64(0)
    lib.kvz_prof_read(name.encode(), ctypes.byref(ms), ctypes.byref(n))
    return ms.value / max(n.value, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ctx", type=int, default=131072)
    ap.add_argument("--from-ratio", type=float, default=0.6)
    ap.add_argument("--ratio", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tighten_bench: needs a GPU (the gather has no CPU implementation)")
    if args.rounds < 5:
        sys.exit("tighten_bench: at least five rounds of each way")
    from kvzip_amd import ops
    from kvzip_amd.kvcache import EvictCache
    lib = ops._lib.load()
    dev, N = "cuda:0", args.ctx
    cfg = types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=H, num_key_value_heads=HKV)
    g = torch.Generator(device=dev).manual_seed(0)
    dense_k = [torch.randn(1, HKV, SINK + N, D, generator=g, device=dev).half() for _ in range(L)]
    dense_v = [torch.randn(1, HKV, SINK + N, D, generator=g, device=dev).half() for _ in range(L)]
    score = [torch.rand(1, HKV, N, generator=g, device=dev).half() for _ in range(L)]

    def cache(ratio=None):
        kv = EvictCache(cfg, (SINK, SINK + N), device=dev, dtype=torch.float16, verbose=False)
        kv.adopt_dense(dense_k, dense_v, SINK + N)
        kv.score = score
        if ratio is not None:
            kv.prune(ratio)
        return kv

    def tighten_staged():
        """The stages of EvictCache.tighten, one by one -> (selection, plan, gather ms, kept rows)."""
        kv = cache(args.from_ratio)
        old_valid, old_plan = kv.valid, kv._plan
        torch.cuda.synchronize()
        lib.kvz_prof_reset()
        t = Timer()
        kv._select(args.ratio, "pair")
        t.mark()
        plan = ops.compact_plan(kv.valid, kv.sink, old_plan.klen, slack=kv.slack)
        meta = torch.cat([plan.meta, ops.mask_resurrects(kv.valid, old_valid)]).cpu()
        t.mark()
        assert int(meta[-1]) == 0
        rows = meta[:L * HKV].view(L, HKV).sum(-1).tolist()
        ops.recompact_layers(kv.key_cache, kv.value_cache, old_plan, old_valid, plan, kv.valid, [r + HKV * kv.slack for r in rows])
        t.mark()
        return t.ms() + [prof_read(lib, "recompact_gather"), sum(rows)]

    def tighten_whole():
        kv = cache(args.from_ratio)
        torch.cuda.synchronize()
        t = Timer()
        kv.tighten(args.ratio)
        t.mark()
        return t.ms()[0]

    def fresh():
        """prepare_init at the small ratio from the dense cache -> (prepare_init ms, its gather kernel ms)."""
        kv = cache()
        kv._select(args.ratio, "pair")
        torch.cuda.synchronize()
        lib.kvz_prof_reset()
        t = Timer()
        kv.prepare_init()
        t.mark()
        return t.ms()[0], prof_read(lib, "compact_gather")

    lib.kvz_prof_enable(1)
    tighten_staged(); tighten_whole(); fresh()      # warm every shape (code objects, allocator)
    rec = {k: [] for k in ("select", "plan", "gather_call", "gather_kernel", "tighten", "fresh_prepare_init", "fresh_gather_kernel")}
    rows = 0
    for _ in range(args.rounds):
        s, p, gc, gk, rows = tighten_staged()
        f, fk = fresh()
        w = tighten_whole()
        for k, v in zip(rec, (s, p, gc, gk, w, f, fk)):
            rec[k].append(v)
    lib.kvz_prof_enable(0)

    def stat(xs):
        m = statistics.median(xs)
        return {"median_ms": round(m, 4), "spread": round((max(xs) - min(xs)) / m, 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}
    moved = 2 * rows * D * 2 * 2                     # read + write, K and V, fp16
    mask = L * HKV * N
    out = {"tool": "tighten_bench", "device": torch.cuda.get_device_name(0), "ctx": N, "from_ratio": args.from_ratio, "ratio": args.ratio,
           "dtype": "float16", "rounds": args.rounds, "kept_rows": rows, "moved_GB": round(moved / 1e9, 3),
           **{k: stat(v) for k, v in rec.items()}}
    out["tighten_gather_TBps"] = round((moved + 2 * mask) / (out["gather_kernel"]["median_ms"] * 1e-3) / 1e12, 3)
    out["fresh_gather_TBps"] = round((moved + mask) / (out["fresh_gather_kernel"]["median_ms"] * 1e-3) / 1e12, 3)
    out["gather_kernel_ratio_tighten_over_fresh"] = round(out["gather_kernel"]["median_ms"] / out["fresh_gather_kernel"]["median_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
