"""Packed-first-step probes over several independent caches whose correct 16-bit output is known EXACTLY (host-only helpers; the
method of tests/multi_probes.py and tests/prefill_probes.py).

A case is one call of ``kvz_multi_prefill``: B independent slack-layout caches, every cache with its own flat K and V, its own segment
starts / base lengths and its own count of rows appended before the call (``offset[b]``), and the queries of the caches back to back:
cache b owns packed positions ``cu_q[b] : cu_q[b + 1]`` (possibly none) with the new K,V rows of those positions.

* Uniform probe: q = 0, every visible key weighs 1.  V marks keys on DISTINCT dims: key j of a segment (base rows, then the rows
  appended before the call, then the run's new rows) on dim j mod (D - 3) - EVERY key, so the keys on both sides of any key-range
  edge are marked -, the rows appended before the call on dim D - 3, the new rows on dim D - 2, and dim D - 1 of every appended /
  new row holds the cache number b + 1 - so a key too many or too few, a key of another cache or a wrong segment start moves an
  output by whole 16-bit steps.  The slack rows behind what a segment holds are ``SLACK_VALUE``.
* Weighted probe: ``SCALE_ONE``, one-hot q (packed position i, group member g of head h selects dim (i*G + g + 5h) mod D), integer K
  in [-spread, 0], V in {0, 1}: every weight is a power of two and every partial and merged sum is exact in fp32.

All caches of a case are carved from ONE K and ONE V allocation (``arena_k`` / ``arena_v``) with ``SLACK_VALUE`` rows between them.
Final normalisation of the combine (kvz_multi_prefill.hip header): out = fp16/bf16(a / l), attn_probes' 'div' form.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

import attn_probes as ap
from multi_probes import _assemble


@dataclass
class MultiPrefillCase:
    q: torch.Tensor                # [Hkv, T, G, D]
    cu_q: List[int]                # B + 1
    arena_k: torch.Tensor          # [rows, D]: every cache's flat K, SLACK_VALUE rows around them
    arena_v: torch.Tensor
    row0: List[int]                # first arena row of cache b
    rows: List[int]                # rows of cache b
    starts: List[List[int]]        # [B][Hkv] segment starts inside cache b
    lens: List[List[int]]          # [B][Hkv] base lengths
    slack: List[int]               # [B] free rows behind every segment
    offset: List[int]              # [B] rows appended before the call
    k_new: torch.Tensor            # [Hkv, T, D]
    v_new: torch.Tensor
    scale: float
    kind: str

    @property
    def dtype(self):
        return self.q.dtype

    @property
    def lengths(self):
        return [self.cu_q[b + 1] - self.cu_q[b] for b in range(len(self.lens))]

    def old(self, b: int, h: int) -> int:
        """keys of segment (b, h) before the call"""
        return self.lens[b][h] + self.offset[b]


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + int(n))
    return cu


def _case(kind, lens, offset, lengths, G, D, dtype, slack, seed, spread=8):
    B, Hkv = len(lens), len(lens[0])
    cu = _cu(lengths)
    T = cu[-1]
    assert len(offset) == B and len(lengths) == B and all(o >= 0 and o + n <= slack for o, n in zip(offset, lengths))
    g = torch.Generator().manual_seed(seed + 1000)
    parts_k, parts_v, starts = [], [], []
    for b in range(B):
        if kind == "uniform":
            p = ap.uniform_probe(lens[b], 1, G, D, dtype, causal=False, slack=slack, seed=seed + b, dense_max=0)   # (layout, random K)
            k, v = p.k.float(), torch.full(p.v.shape, ap.SLACK_VALUE)
            for h, n in enumerate(lens[b]):
                st, o = p.starts[h], offset[b]
                j = torch.arange(n + o)
                v[st:st + n + o] = 0
                v[st + j, j % (D - 3)] = 1
                v[st + n:st + n + o, D - 3] = 1                 # rows appended before the call: marked
                v[st + n:st + n + o, D - 1] = b + 1
        else:
            p = ap.weighted_probe(lens[b], 1, G, D, dtype, causal=False, spread=spread, slack=slack, seed=seed + b, headroom=1)
            k, v = p.k.float(), p.v.float()
            for h, n in enumerate(lens[b]):
                st, o = p.starts[h], offset[b]
                # (always `slack` rows drawn, the first o used: a cache's data does not depend on any cache's offset)
                k[st + n:st + n + o] = -torch.randint(0, spread + 1, (slack, D), generator=g).float()[:o]
                v[st + n:st + n + o] = torch.randint(0, 2, (slack, D), generator=g).float()[:o]
        parts_k.append(k)
        parts_v.append(v)
        starts.append(list(p.starts))
    if kind == "uniform":
        q = torch.zeros(Hkv, T, G, D)
        k_new = torch.randn(Hkv, T, D, generator=g)
        v_new = torch.zeros(Hkv, T, D)
        for b in range(B):
            j = torch.arange(lengths[b])
            for h in range(Hkv):
                v_new[h, cu[b] + j, (lens[b][h] + offset[b] + j) % (D - 3)] = 1
            v_new[:, cu[b]:cu[b + 1], D - 2] = 1
            v_new[:, cu[b]:cu[b + 1], D - 1] = b + 1
        scale = 1.0 / D ** 0.5
    else:
        q = torch.zeros(Hkv, T, G, D)
        for h in range(Hkv):
            r = torch.arange(T * G)
            q[h].view(T * G, D)[r, (r + 5 * h) % D] = 1.0
        k_new = -torch.randint(0, spread + 1, (Hkv, T, D), generator=g).float()
        v_new = torch.randint(0, 2, (Hkv, T, D), generator=g).float()
        scale = ap.SCALE_ONE
    ak, av, row0 = _assemble(parts_k, parts_v, D, dtype)
    return MultiPrefillCase(q.to(dtype), cu, ak, av, row0, [k.shape[0] for k in parts_k], starts, [list(x) for x in lens], [slack] * B,
                            list(offset), k_new.to(dtype), v_new.to(dtype), scale, kind)


def uniform_case(lens, offset, lengths, G, D, dtype, slack=40, seed=0) -> MultiPrefillCase:
    return _case("uniform", lens, offset, lengths, G, D, dtype, slack, seed)


def weighted_case(lens, offset, lengths, G, D, dtype, slack=40, seed=0, spread=8) -> MultiPrefillCase:
    return _case("weighted", lens, offset, lengths, G, D, dtype, slack, seed, spread)


def random_case(lens, offset, lengths, G, D, dtype, slack=40, seed=0) -> MultiPrefillCase:
    g = torch.Generator().manual_seed(seed)
    B, Hkv = len(lens), len(lens[0])
    cu = _cu(lengths)
    T = cu[-1]
    parts_k, parts_v, starts = [], [], []
    for b in range(B):
        st, rows = ap._layout(list(lens[b]), slack)
        parts_k.append(torch.randn(rows, D, generator=g))
        parts_v.append(torch.randn(rows, D, generator=g))
        starts.append(st)
    ak, av, row0 = _assemble(parts_k, parts_v, D, dtype)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
    return MultiPrefillCase(mk(Hkv, T, G, D), cu, ak, av, row0, [k.shape[0] for k in parts_k], starts, [list(x) for x in lens],
                            [slack] * B, list(offset), mk(Hkv, T, D), mk(Hkv, T, D), 1.0 / D ** 0.5, "random")


def row_keys(c: MultiPrefillCase, b: int, h: int, p: int, fault: Optional[str] = None):
    """(K, V) [n, D] (the case's dtype) that packed position cu_q[b] + p of cache b sees at head h: base rows ++ rows appended before
    ++ its run's new rows 0 .. p.  ``fault`` plays a wrong kernel: 'key+1' lets the row see the next new row as well (where the run
    has one), 'foreign' adds the first new row of the next cache that has any."""
    r, c0 = c.row0[b] + c.starts[b][h], c.cu_q[b]
    n = c.old(b, h)
    hi = p + 1
    if fault == "key+1":
        hi = min(p + 2, c.cu_q[b + 1] - c0)
    ks, vs = [c.arena_k[r:r + n], c.k_new[h, c0:c0 + hi]], [c.arena_v[r:r + n], c.v_new[h, c0:c0 + hi]]
    if fault == "foreign":
        B = len(c.lens)
        other = next(o for o in ((b + 1 + i) % B for i in range(B)) if o != b and c.cu_q[o + 1] > c.cu_q[o])
        ks.append(c.k_new[h, c.cu_q[other]:c.cu_q[other] + 1])
        vs.append(c.v_new[h, c.cu_q[other]:c.cu_q[other] + 1])
    return torch.cat(ks), torch.cat(vs)


def expected_out(c: MultiPrefillCase, fault: Optional[str] = None) -> torch.Tensor:
    """[Hkv, T, G, D] in the case's dtype: exact sums, then the combine's a / l and its 16-bit cast."""
    Hkv, T, G, D = c.q.shape
    num = np.zeros((Hkv, T, G, D))
    den = np.zeros((Hkv, T, G))
    for b in range(len(c.lens)):
        for h in range(Hkv):
            n_b = c.cu_q[b + 1] - c.cu_q[b]
            if n_b == 0:
                continue
            # the keys of the run's last position hold those of every earlier one as a prefix (faults: per position)
            for p in range(n_b):
                i = c.cu_q[b] + p
                K, V = row_keys(c, b, h, p, fault)
                K, V = K.double().numpy(), V.double().numpy()
                if c.kind == "uniform":
                    x = np.zeros((G, K.shape[0]))
                else:
                    x = c.q[h, i].double().numpy() @ K.T
                    assert np.array_equal(x, np.round(x))
                P = np.exp2(x - x.max(-1, keepdims=True))
                num[h, i], den[h, i] = P @ V, P.sum(-1)
    return ap.finalize(num, den, c.dtype, "div")


def expected_arenas(c: MultiPrefillCase):
    """(arena_k, arena_v) after the call: the new rows of every cache with positions at seg_start + len + offset + j, every other byte
    as before."""
    ak, av = c.arena_k.clone(), c.arena_v.clone()
    for b in range(len(c.lens)):
        c0, c1 = c.cu_q[b], c.cu_q[b + 1]
        for h in range(len(c.lens[b])):
            r = c.row0[b] + c.starts[b][h] + c.old(b, h)
            ak[r:r + c1 - c0], av[r:r + c1 - c0] = c.k_new[h, c0:c1], c.v_new[h, c0:c1]
    return ak, av


def concat_for_oracle(c: MultiPrefillCase, b: int):
    """Cache b's explicit concatenation (old rows ++ the run's new rows) as one flat ragged cache and its queries:
    (q [Hkv * n_b, G, D], k, v [rows, D], starts, lens) for ``orc.varlen_attn(..., q_len=n_b)``."""
    n_b = c.cu_q[b + 1] - c.cu_q[b]
    ks, vs, starts, lens, acc = [], [], [], [], 0
    for h in range(len(c.lens[b])):
        K, V = row_keys(c, b, h, n_b - 1)
        ks.append(K); vs.append(V); starts.append(acc); lens.append(K.shape[0]); acc += K.shape[0]
    q = c.q[:, c.cu_q[b]:c.cu_q[b + 1]].reshape(-1, c.q.shape[2], c.q.shape[3])
    return q, torch.cat(ks), torch.cat(vs), starts, lens


def as_model_tensors(c: MultiPrefillCase):
    """(query [1, H, T, D], k_new, v_new [1, Hkv, T, D]) as the attention layer hands them over: transposed views of [1, T, heads, D]."""
    Hkv, T, G, D = c.q.shape
    q = c.q.permute(1, 0, 2, 3).reshape(1, T, Hkv * G, D).transpose(1, 2)
    k = c.k_new.transpose(0, 1).reshape(1, T, Hkv, D).contiguous().transpose(1, 2)
    v = c.v_new.transpose(0, 1).reshape(1, T, Hkv, D).contiguous().transpose(1, 2)
    return q, k, v
