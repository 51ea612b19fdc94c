"""Forked-decode probes whose correct 16-bit output is known EXACTLY (host-only helpers; the method of tests/attn_probes.py).

A case is one call of ``kvz_fork_attn_append``: B branches, a shared ragged cache, per-branch tails, one new row per branch.

* Uniform probe: q = 0, every visible key weighs 1.  V marks keys on DISTINCT dims: shared keys on dims [0, D - 3) (attn_probes'
  dense / boundary marking), old tail rows on dim D - 3, the new row on dim D - 2, and dim D - 1 of every tail / new row holds the
  branch number b + 1 - so a key too many or too few, or a key of another branch, moves an output by whole 16-bit steps.  Unused
  tail rows, the slack behind shared segments and the tails of inactive branches hold ``SLACK_VALUE``.
* Weighted probe: ``SCALE_ONE``, one-hot q (row r = b*G + g of head h selects dim (r + 5h) mod D), integer K in [-spread, 0]:
  every weight is a power of two and every partial and merged sum is exact in fp32.

Final normalisation of the fork combine (kvz_fork.hip header): out = fp16/bf16(a / l), attn_probes' 'div' form.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

import attn_probes as ap


def fork_items(tunable_items: int, B: int, Hkv: int, G: int, cus: int = 256) -> int:
    """Work items the shared part of a fork launch is cut into (kvz_fork.hip: fork_items): the decode kernel's count less the tail
    blocks of the same launch, never below a quarter of the CUs (or the knob itself when it is smaller)."""
    t = tunable_items if tunable_items > 0 else (cus - Hkv if Hkv < cus * 3 // 4 else cus // 4)
    n_rtiles = (B * G + 15) // 16
    nt = 2 if n_rtiles >= 2 else 1
    gt = (G + 15) // 16
    n_tail = B * ((gt + nt - 1) // nt) * Hkv
    floor_items = cus // 4
    return t - n_tail if t - n_tail > floor_items else min(t, floor_items)


@dataclass
class ForkCase:
    q: torch.Tensor            # [B, Hkv, G, D]
    k: torch.Tensor            # [rows, D] shared flat cache
    v: torch.Tensor
    starts: List[int]
    lens: List[int]            # keys per head the call sees (k_len + k_len_offset)
    k_len_offset: int
    tail_k: torch.Tensor       # [B, Hkv, cap, D]
    tail_v: torch.Tensor
    tail_len: List[int]        # -1: inactive branch
    k_new: torch.Tensor        # [B, Hkv, 1, D]
    v_new: torch.Tensor
    scale: float
    kind: str

    @property
    def dtype(self):
        return self.q.dtype


def _tails(B, Hkv, cap, D, tail_len, fill_k, fill_v, g):
    tk = torch.full((B, Hkv, cap, D), ap.SLACK_VALUE)
    tv = torch.full((B, Hkv, cap, D), ap.SLACK_VALUE)
    for b, t in enumerate(tail_len):
        if t > 0:
            tk[b, :, :t], tv[b, :, :t] = fill_k(b, t), fill_v(b, t)
    return tk, tv


def uniform_case(lens: Sequence[int], B: int, G: int, D: int, dtype, tail_len: Sequence[int], tail_cap: int, k_len_offset: int = 0,
                 items: Sequence[int] = (), seed: int = 0) -> ForkCase:
    Hkv = len(lens)
    p = ap.uniform_probe(lens, 1, G, D, dtype, causal=False, items=items, slack=3, seed=seed)
    v = p.v.float()
    for h, n in enumerate(lens):
        v[p.starts[h]:p.starts[h] + n, D - 3:] = 0          # the last three dims belong to the tails
    g = torch.Generator().manual_seed(seed + 1)

    def marked(b, t, dim):
        x = torch.zeros(Hkv, t, D)
        x[..., dim] = 1
        x[..., D - 1] = b + 1
        return x
    tk, tv = _tails(B, Hkv, tail_cap, D, tail_len, lambda b, t: torch.randn(Hkv, t, D, generator=g), lambda b, t: marked(b, t, D - 3), g)
    v_new = torch.stack([marked(b, 1, D - 2) for b in range(B)])
    k_new = torch.randn(B, Hkv, 1, D, generator=g)
    q = torch.zeros(B, Hkv, G, D)
    return ForkCase(q.to(dtype), p.k, v.to(dtype), p.starts, list(lens), k_len_offset, tk.to(dtype), tv.to(dtype), list(tail_len),
                    k_new.to(dtype), v_new.to(dtype), p.scale, "uniform")


def weighted_case(lens: Sequence[int], B: int, G: int, D: int, dtype, tail_len: Sequence[int], tail_cap: int, k_len_offset: int = 0,
                  spread: int = 8, seed: int = 0) -> ForkCase:
    Hkv = len(lens)
    assert all(n >= 1 for n in lens), "the weighted probe puts a row maximum of 0 into every shared segment"
    p = ap.weighted_probe(lens, 1, G, D, dtype, causal=False, spread=spread, slack=3, seed=seed, headroom=1)
    g = torch.Generator().manual_seed(seed + 1)
    tk, tv = _tails(B, Hkv, tail_cap, D, tail_len, lambda b, t: -torch.randint(0, spread + 1, (Hkv, t, D), generator=g).float(),
                    lambda b, t: torch.randint(0, 2, (Hkv, t, D), generator=g).float(), g)
    k_new = -torch.randint(0, spread + 1, (B, Hkv, 1, D), generator=g).float()
    v_new = torch.randint(0, 2, (B, Hkv, 1, D), generator=g).float()
    q = torch.zeros(B, Hkv, G, D)
    for h in range(Hkv):
        for b in range(B):
            for gg in range(G):
                q[b, h, gg, (b * G + gg + 5 * h) % D] = 1.0
    return ForkCase(q.to(dtype), p.k, p.v, p.starts, list(lens), k_len_offset, tk.to(dtype), tv.to(dtype), list(tail_len),
                    k_new.to(dtype), v_new.to(dtype), ap.SCALE_ONE, "weighted")


def branch_keys(c: ForkCase, b: int, h: int):
    """(K, V) float64 [n, D] that branch b sees at head h: shared segment ++ tail rows 0 .. tail_len[b] - 1 ++ the new row."""
    st, n, t = c.starts[h], c.lens[h], c.tail_len[b]
    K = torch.cat([c.k[st:st + n], c.tail_k[b, h, :t], c.k_new[b, h]]).double().numpy()
    V = torch.cat([c.v[st:st + n], c.tail_v[b, h, :t], c.v_new[b, h]]).double().numpy()
    return K, V


def expected_out(c: ForkCase) -> torch.Tensor:
    """[B, Hkv, G, D] in the case's dtype: exact sums, then the combine's a / l and its 16-bit cast; inactive branches zero."""
    B, Hkv, G, D = c.q.shape
    num = np.zeros((B, Hkv, G, D))
    den = np.zeros((B, Hkv, G))
    for b in range(B):
        if c.tail_len[b] < 0:
            continue
        for h in range(Hkv):
            K, V = branch_keys(c, b, h)
            if c.kind == "uniform":
                x = np.zeros((G, K.shape[0]))
            else:
                x = c.q[b, h].double().numpy() @ K.T
                assert np.array_equal(x, np.round(x))
            P = np.exp2(x - x.max(-1, keepdims=True))
            num[b, h], den[b, h] = P @ V, P.sum(-1)
    return ap.finalize(num, den, c.dtype, "div")


def expected_tails(c: ForkCase):
    """(tail_k, tail_v) after the call: the new rows of the active branches at tail[b, :, tail_len[b]], every other byte as before."""
    tk, tv = c.tail_k.clone(), c.tail_v.clone()
    for b, t in enumerate(c.tail_len):
        if t >= 0:
            tk[b, :, t], tv[b, :, t] = c.k_new[b, :, 0], c.v_new[b, :, 0]
    return tk, tv


def concat_for_oracle(c: ForkCase, b: int):
    """Branch b's explicit concatenation as one flat ragged cache: (k, v [rows, D], starts, lens) for ``orc.varlen_attn``."""
    Hkv = c.q.shape[1]
    ks, vs, starts, lens, acc = [], [], [], [], 0
    for h in range(Hkv):
        st, n, t = c.starts[h], c.lens[h], c.tail_len[b]
        kh = torch.cat([c.k[st:st + n], c.tail_k[b, h, :t], c.k_new[b, h]])
        vh = torch.cat([c.v[st:st + n], c.tail_v[b, h, :t], c.v_new[b, h]])
        ks.append(kh); vs.append(vh); starts.append(acc); lens.append(kh.shape[0]); acc += kh.shape[0]
    return torch.cat(ks), torch.cat(vs), starts, lens


def random_case(lens: Sequence[int], B: int, G: int, D: int, dtype, tail_len: Sequence[int], tail_cap: int, k_len_offset: int = 0,
                seed: int = 0) -> ForkCase:
    g = torch.Generator().manual_seed(seed)
    Hkv = len(lens)
    starts, rows = ap._layout(list(lens), 3)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
    return ForkCase(mk(B, Hkv, G, D), mk(rows, D), mk(rows, D), starts, list(lens), k_len_offset, mk(B, Hkv, tail_cap, D),
                    mk(B, Hkv, tail_cap, D), list(tail_len), mk(B, Hkv, 1, D), mk(B, Hkv, 1, D), 1.0 / D ** 0.5, "random")
