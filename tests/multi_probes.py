"""Batched-decode probes whose correct 16-bit output is known EXACTLY (host-only helpers; the method of tests/attn_probes.py).

A case is one call of ``kvz_multi_attn_append``: B independent slack-layout caches, every cache with its own flat K and V, its own
segment starts / base lengths and its own count of rows appended before the call (``offset[b]``; -1 = inactive), one new row per cache.

* Uniform probe: q = 0, every visible key weighs 1.  V marks keys on DISTINCT dims: the base rows on dims [0, D - 3) (attn_probes'
  dense / boundary marking), the rows appended before the call on dim D - 3, the new row on dim D - 2, and dim D - 1 of every appended /
  new row holds the cache number b + 1 - so a key too many or too few, a key of another cache or a wrong segment start moves an output
  by whole 16-bit steps.  The slack rows behind what a segment holds are ``SLACK_VALUE``.
* Weighted probe: ``SCALE_ONE``, one-hot q, integer K in [-spread, 0]: every weight is a power of two and every partial and merged sum
  is exact in fp32.

All caches of a case are carved from ONE K and ONE V allocation (``arena_k`` / ``arena_v``) with ``SLACK_VALUE`` rows between them:
what a cache's neighbours hold is then known too.  Final normalisation of the combine (kvz_multi.hip header): out = fp16/bf16(a / l),
attn_probes' 'div' form.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

import attn_probes as ap

GAP_ROWS = 8        # SLACK_VALUE rows before, between and behind the caches of a case


def multi_items(tunable_items: int, S: int, cus: int = 256) -> int:
    """Work items a step is cut into (kvz_multi.hip: multi_items): the decode kernel's rule with S = B * Hkv segments."""
    return tunable_items if tunable_items > 0 else (cus - S if S < cus * 3 // 4 else cus // 4)


@dataclass
class MultiCase:
    q: torch.Tensor                # [B, Hkv, G, D]
    arena_k: torch.Tensor          # [rows, D]: every cache's flat K, SLACK_VALUE rows around them
    arena_v: torch.Tensor
    row0: List[int]                # first arena row of cache b
    rows: List[int]                # rows of cache b
    starts: List[List[int]]        # [B][Hkv] segment starts inside cache b
    lens: List[List[int]]          # [B][Hkv] base lengths
    slack: List[int]               # [B] free rows behind every segment
    offset: List[int]              # [B] rows appended before the call; -1: inactive
    k_new: torch.Tensor            # [B, Hkv, 1, D]
    v_new: torch.Tensor
    scale: float
    kind: str

    @property
    def dtype(self):
        return self.q.dtype

    def seen(self, b: int, h: int) -> int:
        """keys of segment (b, h) before the call"""
        return self.lens[b][h] + max(self.offset[b], 0)

    def segment_lengths(self) -> List[int]:
        """what the launch cuts its work items from: len + offset + 1 of every segment of a live cache"""
        return [self.seen(b, h) + 1 for b in range(len(self.lens)) if self.offset[b] >= 0 for h in range(len(self.lens[b]))]


def _assemble(parts_k, parts_v, D, dtype):
    """caches [(k [rows, D], v)] -> one arena each with GAP_ROWS of SLACK_VALUE around every cache"""
    gap = torch.full((GAP_ROWS, D), ap.SLACK_VALUE)
    ks, vs, row0, acc = [gap], [gap], [], GAP_ROWS
    for k, v in zip(parts_k, parts_v):
        row0.append(acc)
        ks += [k.float(), gap]
        vs += [v.float(), gap]
        acc += k.shape[0] + GAP_ROWS
    return torch.cat(ks).to(dtype), torch.cat(vs).to(dtype), row0


def _case(kind, lens, offset, G, D, dtype, slack, items, seed, spread=8):
    B, Hkv = len(lens), len(lens[0])
    live_off = [max(o, 0) for o in offset]
    assert all(o + 1 <= slack for o in live_off)
    seg_lens = [lens[b][h] + live_off[b] + 1 for b in range(B) for h in range(Hkv)]
    g = torch.Generator().manual_seed(seed + 1000)
    parts_k, parts_v, starts, qs = [], [], [], []
    for b in range(B):
        if kind == "uniform":
            p = ap.uniform_probe(lens[b], 1, G, D, dtype, causal=False, items=items, slack=slack, seed=seed + b, marks_lens=seg_lens)
            k, v = p.k.float(), p.v.float()
            for h, n in enumerate(lens[b]):
                st = p.starts[h]
                v[st:st + n, D - 3:] = 0                       # the last three dims belong to the appended rows
                for i in range(live_off[b]):                    # rows appended before the call: marked
                    v[st + n + i] = 0
                    v[st + n + i, D - 3] = 1
                    v[st + n + i, D - 1] = b + 1
            qs.append(torch.zeros(Hkv, G, D))
        else:
            p = ap.weighted_probe(lens[b], 1, G, D, dtype, causal=False, spread=spread, slack=slack, seed=seed + b, headroom=1)
            k, v = p.k.float(), p.v.float()
            for h, n in enumerate(lens[b]):
                st = p.starts[h]
                o = live_off[b]
                # (always `slack` rows drawn, the first o used: a cache's data does not depend on any cache's offset)
                k[st + n:st + n + o] = -torch.randint(0, spread + 1, (slack, D), generator=g).float()[:o]
                v[st + n:st + n + o] = torch.randint(0, 2, (slack, D), generator=g).float()[:o]
            qs.append(p.q.float().view(Hkv, G, D).roll(b, dims=-1))    # (another dim per cache)
        parts_k.append(k)
        parts_v.append(v)
        starts.append(list(p.starts))
    if kind == "uniform":
        k_new = torch.randn(B, Hkv, 1, D, generator=g)
        v_new = torch.zeros(B, Hkv, 1, D)
        v_new[..., D - 2] = 1
        v_new[..., D - 1] = torch.arange(1, B + 1).view(B, 1, 1).float()
        scale = 1.0 / D ** 0.5
    else:
        k_new = -torch.randint(0, spread + 1, (B, Hkv, 1, D), generator=g).float()
        v_new = torch.randint(0, 2, (B, Hkv, 1, D), generator=g).float()
        scale = ap.SCALE_ONE
    ak, av, row0 = _assemble(parts_k, parts_v, D, dtype)
    return MultiCase(torch.stack(qs).to(dtype), ak, av, row0, [k.shape[0] for k in parts_k], starts, [list(x) for x in lens],
                     [slack] * B, list(offset), k_new.to(dtype), v_new.to(dtype), scale, kind)


def uniform_case(lens, offset, G, D, dtype, slack=8, items: Sequence[int] = (), seed=0) -> MultiCase:
    return _case("uniform", lens, offset, G, D, dtype, slack, items, seed)


def weighted_case(lens, offset, G, D, dtype, slack=8, seed=0, spread=8) -> MultiCase:
    return _case("weighted", lens, offset, G, D, dtype, slack, (), seed, spread)


def random_case(lens, offset, G, D, dtype, slack=8, seed=0) -> MultiCase:
    g = torch.Generator().manual_seed(seed)
    B, Hkv = len(lens), len(lens[0])
    parts_k, parts_v, starts = [], [], []
    for b in range(B):
        st, rows = ap._layout(list(lens[b]), slack)
        parts_k.append(torch.randn(rows, D, generator=g))
        parts_v.append(torch.randn(rows, D, generator=g))
        starts.append(st)
    ak, av, row0 = _assemble(parts_k, parts_v, D, dtype)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
    return MultiCase(mk(B, Hkv, G, D), ak, av, row0, [k.shape[0] for k in parts_k], starts, [list(x) for x in lens], [slack] * B,
                     list(offset), mk(B, Hkv, 1, D), mk(B, Hkv, 1, D), 1.0 / D ** 0.5, "random")


def segment_keys(c: MultiCase, b: int, h: int):
    """(K, V) [n, D] (the case's dtype) that cache b sees at head h: base rows ++ rows appended before ++ the new row."""
    r = c.row0[b] + c.starts[b][h]
    n = c.seen(b, h)
    return torch.cat([c.arena_k[r:r + n], c.k_new[b, h]]), torch.cat([c.arena_v[r:r + n], c.v_new[b, h]])


def expected_out(c: MultiCase) -> torch.Tensor:
    """[B, Hkv, G, D] in the case's dtype: exact sums, then the combine's a / l and its 16-bit cast; inactive caches zero."""
    B, Hkv, G, D = c.q.shape
    num = np.zeros((B, Hkv, G, D))
    den = np.zeros((B, Hkv, G))
    for b in range(B):
        if c.offset[b] < 0:
            continue
        for h in range(Hkv):
            K, V = segment_keys(c, b, h)
            K, V = K.double().numpy(), V.double().numpy()
            if c.kind == "uniform":
                x = np.zeros((G, K.shape[0]))
            else:
                x = c.q[b, h].double().numpy() @ K.T
                assert np.array_equal(x, np.round(x))
            P = np.exp2(x - x.max(-1, keepdims=True))
            num[b, h], den[b, h] = P @ V, P.sum(-1)
    return ap.finalize(num, den, c.dtype, "div")


def expected_arenas(c: MultiCase):
    """(arena_k, arena_v) after the call: the new rows of the live caches at seg_start + len + offset, every other byte as before."""
    ak, av = c.arena_k.clone(), c.arena_v.clone()
    for b, off in enumerate(c.offset):
        if off < 0:
            continue
        for h in range(len(c.lens[b])):
            r = c.row0[b] + c.starts[b][h] + c.lens[b][h] + off
            ak[r], av[r] = c.k_new[b, h, 0], c.v_new[b, h, 0]
    return ak, av


def concat_for_oracle(c: MultiCase, b: int):
    """Cache b's explicit concatenation as one flat ragged cache: (k, v [rows, D], starts, lens) for ``orc.varlen_attn``."""
    ks, vs, starts, lens, acc = [], [], [], [], 0
    for h in range(len(c.lens[b])):
        K, V = segment_keys(c, b, h)
        ks.append(K); vs.append(V); starts.append(acc); lens.append(K.shape[0]); acc += K.shape[0]
    return torch.cat(ks), torch.cat(vs), starts, lens
