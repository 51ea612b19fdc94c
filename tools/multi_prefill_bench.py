#!/usr/bin/env python
"""Packed first step over several independent pruned caches against the per-cache first steps: the attention part of the FIRST steps
(the query tokens) of a wave of B users, each with a cache of its own, over all layers.

  packed     CacheBatch.select_packed + first_step    - per layer ONE kvz_multi_prefill (split + combine launch) for all B caches
  per cache  EvictCache.update + prepare + attend     - per layer and cache kvz_append_inplace and kvz_varlen_attn (-> kvz_flash_fwd,
                                                        often with its split-merge launch): what generate_multi did before

Both in one process, the packed way on B pruned caches and the per-cache way on clones of them (Qwen2.5-7B geometry, ratio 0.3, built
like tools/fork_decode_bench.py builds its cache), on the same inputs, alternating rounds, hipEvent-timed, every shape warmed first;
the caches are sliced back before every pass.  Shapes: N in {8 192, 32 768, 131 072} x B in {2, 4, 8} x {16, 48, 160} query tokens,
and one mixed wave (131 072 + 3 x 8 192).  Prints per shape the median ms per wave of both ways, the ratio, the spread of the rounds
((max - min) / median) and `slower_beyond_spread` (every packed round slower than every per-cache round), then ONE JSON line.
Needs a GPU: there is no fallback.

Without --ctx / --mixed this is the driver: one child process per context length, each GPU step under a time limit of its own
(`timeout -k 10`), chained - it stops at the first step that fails:

    python tools/multi_prefill_bench.py [--rounds 5] [--iters 3] [--limit 900] [--out profiles/multi_prefill_ab.txt]
    timeout -k 10 600 python tools/multi_prefill_bench.py --ctx 32768        # one step by hand
    timeout -k 10 600 python tools/multi_prefill_bench.py --mixed
"""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

L, H, HKV, D = 28, 28, 4, 128           # Qwen2.5-7B
CTXS = (8192, 32768, 131072)
BS = (2, 4, 8)
TOKENS = (16, 48, 160)
MIXED = (131072, 8192, 8192, 8192)


def clone_cache(kv):
    """A pruned slack-layout cache with rows of its own and the same (read-only) segment tables."""
    c = copy.copy(kv)
    c._async, c._score_ws = -1, []          # (the copy owns no scoring stream and no scoring workspace: nothing to release)
    c.key_cache = [t.clone() for t in kv.key_cache]
    c.value_cache = [t.clone() for t in kv.value_cache]
    c.info = {k: (list(v) if isinstance(v, list) else v) for k, v in kv.info.items()}
    c._attn_ws_cache = None
    return c


def measure(kvs, clones, lengths, rounds, iters, dev):
    import torch
    from fork_decode_bench import timed
    from kvzip_amd.kvcache import CacheBatch
    B, T = len(kvs), sum(lengths)
    g = torch.Generator(device=dev).manual_seed(B * 1000 + T)
    # [1, H, T, D] views of [1, T, H, D] storage, as the projections hand them over
    q = [torch.randn(1, T, H, D, generator=g, device=dev).half().transpose(1, 2) for _ in range(L)]
    k = [torch.randn(1, T, HKV, D, generator=g, device=dev).half().transpose(1, 2) for _ in range(L)]
    v = [torch.randn(1, T, HKV, D, generator=g, device=dev).half().transpose(1, 2) for _ in range(L)]
    batch = CacheBatch(kvs)
    seen = [c.get_seq_length() for c in kvs]
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)

    def packed():
        for c, s in zip(kvs, seen):
            c.slice(s)
        batch.select_packed(list(range(B)), lengths)
        for l in range(L):
            batch.first_step(q[l], k[l], v[l], l)

    def per_cache():
        for b, c in enumerate(clones):
            c.slice(seen[b])
            sl = slice(cu[b], cu[b + 1])
            for l in range(L):
                kc, vc = c.update(k[l][:, :, sl], v[l][:, :, sl], l)
                qq, kk, vv, info = c.prepare(q[l][:, :, sl].contiguous(), kc, vc, l)
                c.attend(qq, kk, vv, info, causal=True)

    packed(); per_cache(); packed(); per_cache()      # warm both shapes (workspaces, tables, code objects)
    torch.cuda.synchronize()
    same = all(torch.equal(a.key_cache[l], b.key_cache[l]) and torch.equal(a.value_cache[l], b.value_cache[l])
               for a, b in zip(kvs, clones) for l in (0, L - 1))
    tp, tc = [], []
    for _ in range(rounds):
        tp.append(timed(packed, iters))
        tc.append(timed(per_cache, iters))
    mp, mc = statistics.median(tp), statistics.median(tc)
    return {"B": B, "tokens": lengths[0] if len(set(lengths)) == 1 else lengths, "packed_ms_per_wave": round(mp, 4),
            "per_cache_ms_per_wave": round(mc, 4), "ratio": round(mc / mp, 3), "packed_spread": round((max(tp) - min(tp)) / mp, 4),
            "per_cache_spread": round((max(tc) - min(tc)) / mc, 4), "slower_beyond_spread": bool(min(tp) > max(tc)),
            "rows_identical": bool(same), "rounds": rounds, "iters": iters}


def table(title, rows):
    out = [title, f"{'B':>3} {'tokens':>6} {'packed':>10} {'per cache':>10} {'ratio':>7} {'spread p':>9} {'spread c':>9}  slower_beyond_spread"]
    for r in rows:
        tok = r["tokens"] if isinstance(r["tokens"], int) else "mixed"
        out.append(f"{r['B']:>3} {tok:>6} {r['packed_ms_per_wave']:>10.3f} {r['per_cache_ms_per_wave']:>10.3f} {r['ratio']:>7.2f} "
                   f"{r['packed_spread']:>9.3f} {r['per_cache_spread']:>9.3f}  {r['slower_beyond_spread']}")
    return "\n".join(out)


def step(args):
    """One GPU step: the shapes of one context length, or the mixed wave."""
    import torch
    from fork_decode_bench import build_cache
    if not torch.cuda.is_available():
        sys.exit("multi_prefill_bench: needs a GPU (the packed first step has no CPU implementation)")
    dev = "cuda:0"
    if args.mixed:
        bases = {n: build_cache(L, H, HKV, D, n, args.ratio, dev) for n in sorted(set(MIXED))}
        kvs = [clone_cache(bases[n]) for n in MIXED]
        clones = [clone_cache(bases[n]) for n in MIXED]
        rows = [measure(kvs, clones, [n] * len(MIXED), args.rounds, args.iters, dev) for n in (48,)]
        for r in rows:
            r["tokens"] = [r["tokens"]] * len(MIXED)
        title = f"qwen2.5-7b  ctx {'+'.join(str(n) for n in MIXED)}  ratio {args.ratio}  fp16  48 tokens each"
        ctx = list(MIXED)
    else:
        base = build_cache(L, H, HKV, D, args.ctx, args.ratio, dev)
        kvs = [base] + [clone_cache(base) for _ in range(max(BS) - 1)]
        clones = [clone_cache(base) for _ in range(max(BS))]
        rows = [measure(kvs[:B], clones[:B], [n] * B, args.rounds, args.iters, dev) for n in TOKENS for B in BS]
        title = f"qwen2.5-7b  ctx {args.ctx}  ratio {args.ratio}  fp16  (ms per wave: attention of the first steps, {L} layers)"
        ctx = args.ctx
    print(table(title, rows))
    print(json.dumps({"tool": "multi_prefill_bench", "device": torch.cuda.get_device_name(0), "geometry": "qwen2.5-7b", "ctx": ctx,
                      "ratio": args.ratio, "dtype": "float16", "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=None)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=900, help="seconds every GPU step may take (driver)")
    ap.add_argument("--out", default=None, help="also write the tables to this file (driver)")
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("multi_prefill_bench: at least five rounds of each way")
    if args.ctx is not None or args.mixed:
        return step(args)
    # the driver: every GPU step a process of its own under its own time limit, chained; the first failure ends the run
    text = []
    for extra in [["--ctx", str(n)] for n in CTXS] + [["--mixed"]]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds),
               "--iters", str(args.iters), "--ratio", str(args.ratio)] + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(f"multi_prefill_bench: step {' '.join(extra)} ended with status {r.returncode}: nothing more is started")
        text.append("\n".join(x for x in r.stdout.splitlines() if not x.startswith("{")))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n\n".join(text) + "\n")


if __name__ == "__main__":
    main()
