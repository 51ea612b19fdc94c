"""Verify-step probes whose correct 16-bit output is known EXACTLY (host-only helpers; the method of tests/attn_probes.py and
tests/fork_probes.py).

A case is one call of ``kvz_spec_attn_append``: t consecutive new positions of one sequence on a ragged slack-layout cache.  Query row
(p, g) of head h sees the ``old`` rows of the head's segment, unmasked, and the new rows 0 .. p.

* Uniform probe: q = 0, every visible key weighs 1.  V marks keys on DISTINCT dims: old rows on dims [0, D - t) (attn_probes' dense /
  boundary marking), new row p on dim D - t + p - so a key too many (the slack behind a segment holds ``SLACK_VALUE``), a key of a later
  position or a missing new row moves an output by whole 16-bit steps.
* Weighted probe: ``SCALE_ONE``, one-hot q (row r = p*G + g of head h selects dim (r + 5h) mod D), integer K in [-spread, 0]: every
  weight is a power of two and every partial and merged sum is exact in fp32.

Final normalisation of the combine (kvz_spec.hip header): out = fp16/bf16(a / l), attn_probes' 'div' form.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

import attn_probes as ap


def spec_items(tunable_items: int, Hkv: int, cus: int = 256) -> int:
    """Work items the shared part of a verify launch is cut into (kvz_spec.hip: spec_items): the decode kernel's count less the Hkv
    triangle items of the same launch, never below a quarter of the CUs (or the knob itself when it is smaller)."""
    t = tunable_items if tunable_items > 0 else (cus - Hkv if Hkv < cus * 3 // 4 else cus // 4)
    floor_items = cus // 4
    return t - Hkv if t - Hkv > floor_items else min(t, floor_items)


@dataclass
class SpecCase:
    q: torch.Tensor            # [Hkv, t, G, D]
    k: torch.Tensor            # [rows, D] flat cache, `slack` free rows behind every segment
    v: torch.Tensor
    starts: List[int]
    lens: List[int]            # rows per head the call sees before it appends (k_len + k_len_offset)
    k_len_offset: int
    slack: int                 # free rows behind lens[h] (the call's `slack` argument is k_len_offset + slack)
    k_new: torch.Tensor        # [Hkv, t, D]
    v_new: torch.Tensor
    scale: float
    kind: str

    @property
    def dtype(self):
        return self.q.dtype

    @property
    def t(self):
        return self.q.shape[1]


def uniform_case(lens: Sequence[int], t: int, G: int, D: int, dtype, k_len_offset: int = 0, items: Sequence[int] = (),
                 seed: int = 0) -> SpecCase:
    Hkv = len(lens)
    assert t < D
    slack = t + 2
    p = ap.uniform_probe(lens, 1, G, D, dtype, causal=False, items=items, slack=slack, seed=seed)
    v = p.v.float()
    for h, n in enumerate(lens):
        v[p.starts[h]:p.starts[h] + n, D - t:] = 0          # the last t dims belong to the new rows
    g = torch.Generator().manual_seed(seed + 1)
    v_new = torch.zeros(Hkv, t, D)
    v_new[:, torch.arange(t), D - t + torch.arange(t)] = 1
    k_new = torch.randn(Hkv, t, D, generator=g)
    q = torch.zeros(Hkv, t, G, D)
    return SpecCase(q.to(dtype), p.k, v.to(dtype), p.starts, list(lens), k_len_offset, slack, k_new.to(dtype), v_new.to(dtype),
                    p.scale, "uniform")


def weighted_case(lens: Sequence[int], t: int, G: int, D: int, dtype, k_len_offset: int = 0, spread: int = 8,
                  seed: int = 0) -> SpecCase:
    Hkv = len(lens)
    slack = t + 2
    p = ap.weighted_probe(lens, 1, G, D, dtype, causal=False, spread=spread, slack=slack, seed=seed, headroom=1)
    g = torch.Generator().manual_seed(seed + 1)
    k_new = -torch.randint(0, spread + 1, (Hkv, t, D), generator=g).float()
    v_new = torch.randint(0, 2, (Hkv, t, D), generator=g).float()
    q = torch.zeros(Hkv, t * G, D)
    r = torch.arange(t * G)
    for h in range(Hkv):
        q[h, r, (r + 5 * h) % D] = 1.0
    return SpecCase(q.view(Hkv, t, G, D).to(dtype), p.k, p.v, p.starts, list(lens), k_len_offset, slack, k_new.to(dtype),
                    v_new.to(dtype), ap.SCALE_ONE, "weighted")


def random_case(lens: Sequence[int], t: int, G: int, D: int, dtype, k_len_offset: int = 0, seed: int = 0) -> SpecCase:
    g = torch.Generator().manual_seed(seed)
    Hkv = len(lens)
    slack = t + 2
    starts, rows = ap._layout(list(lens), slack)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
    return SpecCase(mk(Hkv, t, G, D), mk(rows, D), mk(rows, D), starts, list(lens), k_len_offset, slack, mk(Hkv, t, D), mk(Hkv, t, D),
                    1.0 / D ** 0.5, "random")


def expected_out(c: SpecCase) -> torch.Tensor:
    """[Hkv, t, G, D] in the case's dtype: exact sums, then the combine's a / l and its 16-bit cast."""
    Hkv, t, G, D = c.q.shape
    num = np.zeros((Hkv, t, G, D))
    den = np.zeros((Hkv, t, G))
    for h in range(Hkv):
        st, n = c.starts[h], c.lens[h]
        for p in range(t):
            K = torch.cat([c.k[st:st + n], c.k_new[h, :p + 1]]).double().numpy()
            V = torch.cat([c.v[st:st + n], c.v_new[h, :p + 1]]).double().numpy()
            if c.kind == "uniform":
                x = np.zeros((G, K.shape[0]))
            else:
                x = c.q[h, p].double().numpy() @ K.T
                assert np.array_equal(x, np.round(x))
            P = np.exp2(x - x.max(-1, keepdims=True))
            num[h, p], den[h, p] = P @ V, P.sum(-1)
    return ap.finalize(num, den, c.dtype, "div")


def expected_cache(c: SpecCase):
    """(k, v) after the call: the t new rows behind every segment, every other byte as before."""
    k, v = c.k.clone(), c.v.clone()
    for h in range(len(c.lens)):
        r = c.starts[h] + c.lens[h]
        k[r:r + c.t], v[r:r + c.t] = c.k_new[h], c.v_new[h]
    return k, v


def concat_for_oracle(c: SpecCase):
    """The segments with the new rows behind them as one flat ragged cache: (k, v [rows, D], starts, lens) for ``orc.varlen_attn``
    with q_len = t and the bottom-right causal mask."""
    ks, vs, starts, lens, acc = [], [], [], [], 0
    for h in range(len(c.lens)):
        st, n = c.starts[h], c.lens[h]
        ks += [c.k[st:st + n], c.k_new[h]]
        vs += [c.v[st:st + n], c.v_new[h]]
        starts.append(acc); lens.append(n + c.t); acc += n + c.t
    return torch.cat(ks), torch.cat(vs), starts, lens
