"""Host-only helpers of the indexed-attention tests (kvz_retain_attn, include/kvzip_hip_retain.h): a probe of tests/attn_probes.py
- compact K, V per head, head lengths, exactly known output - scattered into a DENSE ``[Hkv, capacity, D]`` store under a mask, with the
index of kept positions built HERE on the host (torch.nonzero), so that the attention tests do not depend on the index kernel.

Every evicted row and every row at or behind ``fill`` holds NaN in both K and V: a kernel that reads one of them returns NaN.

Layout of head h (``sink`` rows, ``N`` context rows under ``masks[h]``, ``tail`` rows behind the context):
    key j <  n_h = sink + kept_h  ->  position idx[start_h + j]
    key j >= n_h                  ->  position ctx_end + (j - n_h),   ctx_end = sink + N
so the probe's head h has n_h + tail keys, in this order."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Sequence

import torch

import attn_probes as ap

MASK_KINDS = ("all", "none", "random", "runs")


def make_masks(N: int, seed: int = 0, kinds: Sequence[str] = MASK_KINDS, random_kept: int = -1) -> List[torch.Tensor]:
    """One bool ``[N]`` mask per head: everything kept; nothing kept (sink and tail only); random 0.3 (``random_kept`` >= 0: exactly
    that many kept); runs of 33 kept / 31 dropped, so that runs of consecutive positions straddle the 32-key tiles unaligned."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for kind in kinds:
        if kind == "all":
            m = torch.ones(N, dtype=torch.bool)
        elif kind == "none":
            m = torch.zeros(N, dtype=torch.bool)
        elif kind == "random":
            if random_kept >= 0:
                m = torch.zeros(N, dtype=torch.bool)
                m[torch.randperm(N, generator=g)[:random_kept]] = True
            else:
                m = torch.rand(N, generator=g) < 0.3
        elif kind == "runs":
            m = (torch.arange(N) % 64) < 33
        else:
            raise ValueError(kind)
        out.append(m)
    return out


def head_lens(masks: Sequence[torch.Tensor], sink: int, tail: int) -> List[int]:
    """Keys per head: sink + kept + tail."""
    return [sink + int(m.sum()) + tail for m in masks]


@dataclass
class Dense:
    k: torch.Tensor            # [Hkv, capacity, D] 16-bit (CPU), NaN wherever no kept row lies
    v: torch.Tensor
    idx: torch.Tensor          # int32 [max(total, 1)]: the kept positions of the heads back to back
    starts: List[int]
    counts: List[int]
    ctx_end: int
    fill: int                  # rows in use per head

    @property
    def meta(self):
        Hkv = len(self.counts)
        return (C.c_int32 * (2 * Hkv))(*self.starts, *self.counts)


def scatter(p: ap.Probe, masks: Sequence[torch.Tensor], sink: int, tail: int, spare: int = 9) -> Dense:
    """The rows of probe ``p`` (head h: ``sink + kept_h + tail`` keys from ``p.starts[h]`` on) where a dense cache holds them."""
    Hkv, N, D = len(masks), masks[0].numel(), p.k.shape[1]
    ctx_end = sink + N
    fill = ctx_end + tail
    cap = fill + spare
    k = torch.full((Hkv, cap, D), float("nan"), dtype=p.k.dtype)
    v = torch.full((Hkv, cap, D), float("nan"), dtype=p.v.dtype)
    idx, starts, counts, o = [], [], [], 0
    for h, m in enumerate(masks):
        pos = torch.nonzero(torch.cat([torch.ones(sink, dtype=torch.bool), m])).flatten()
        n = pos.numel()
        assert p.lens[h] == n + tail, (h, p.lens[h], n, tail)
        st = p.starts[h]
        k[h, pos], v[h, pos] = p.k[st:st + n], p.v[st:st + n]
        k[h, ctx_end:fill], v[h, ctx_end:fill] = p.k[st + n:st + n + tail], p.v[st + n:st + n + tail]
        idx.append(pos.to(torch.int32))
        starts.append(o)
        counts.append(n)
        o += n
    idx = torch.cat(idx) if o else torch.zeros(1, dtype=torch.int32)
    return Dense(k, v, idx, starts, counts, ctx_end, fill)


def split_last(d: Dense):
    """The store BEFORE the last row of every head was appended (that row NaN again, fill - 1 rows in use) and the row itself as a
    decode step hands it over: K ``[1, Hkv, 1, D]`` contiguous, V a strided view of a ``[1, 1, Hkv*D]`` projection output."""
    Hkv, _, D = d.k.shape
    r = d.fill - 1
    k_new = d.k[:, r].clone().view(1, Hkv, 1, D)
    v_new = d.v[:, r].clone().view(1, 1, Hkv, D).transpose(1, 2)
    k, v = d.k.clone(), d.v.clone()
    k[:, r] = float("nan")
    v[:, r] = float("nan")
    return Dense(k, v, d.idx, d.starts, d.counts, d.ctx_end, r), k_new, v_new


def random_probe(lens: Sequence[int], q_len: int, G: int, D: int, dtype, seed: int = 0) -> ap.Probe:
    """Random data in the probe's flat layout WITHOUT slack: ``k`` / ``v`` are the compacted copy the gather route attends over."""
    g = torch.Generator().manual_seed(seed)
    lens = [int(n) for n in lens]
    starts, rows = ap._layout(lens, 0)
    Hkv = len(lens)
    q = torch.randn(Hkv * q_len, G, D, generator=g)
    k = torch.randn(rows, D, generator=g)
    v = torch.randn(rows, D, generator=g)
    return ap.Probe(q.to(dtype), k.to(dtype), v.to(dtype), starts, lens, q_len, True, 1.0 / math.sqrt(D), "random", {})
