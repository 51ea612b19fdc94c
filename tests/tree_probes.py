"""Tree verify-step probes whose correct 16-bit output is known EXACTLY (host-only helpers; the cases of tests/spec_probes.py with a
tree among the new rows).

A case is one call of ``kvz_tree_attn_append``: the t new positions are the nodes of a tree given by its parent vector (node 0 the
root, ``parents[i] < i``).  Query row (p, g) of head h sees the ``old`` rows of the head's segment, unmasked, and the new rows of node
p's ancestors and of p itself.  The uniform probe marks new row j on its own V dim, so an output shows exactly which new keys a row
saw; the weighted probe keeps every partial and merged sum exact in fp32 (see spec_probes).
"""
from __future__ import annotations

import random
from typing import List

import numpy as np
import torch

import attn_probes as ap
import spec_probes as sp

KINDS = ("chain", "star", "interleaved", "random")


def parents_of(kind: str, t: int, seed: int = 0) -> List[int]:
    """chain: i - 1; star: every node a child of the root; interleaved: two chains, parent i - 2 (node 1 continues the root);
    random: parent uniform in [0, i), seeded."""
    if kind == "chain":
        return [-1] + list(range(t - 1))
    if kind == "star":
        return [-1] + [0] * (t - 1)
    if kind == "interleaved":
        return [-1] + [max(i - 2, 0) for i in range(1, t)]
    assert kind == "random"
    rng = random.Random(1000 * t + seed)
    return [-1] + [rng.randrange(i) for i in range(1, t)]


def visible(parents: List[int]) -> List[List[int]]:
    """Per node the ascending list of new rows it sees: its ancestors and itself (computed by walking up, not through the masks the
    code under test takes)."""
    out = []
    for p in range(len(parents)):
        seen, x = [], p
        while x >= 0:
            seen.append(x)
            x = parents[x]
        out.append(sorted(seen))
    return out


def expected_out(c: sp.SpecCase, parents: List[int]) -> torch.Tensor:
    """[Hkv, t, G, D] in the case's dtype: exact sums over the old rows and the ancestor rows, then the combine's a / l and its cast."""
    Hkv, t, G, D = c.q.shape
    vis = visible(parents)
    num = np.zeros((Hkv, t, G, D))
    den = np.zeros((Hkv, t, G))
    for h in range(Hkv):
        st, n = c.starts[h], c.lens[h]
        for p in range(t):
            K = torch.cat([c.k[st:st + n], c.k_new[h, vis[p]]]).double().numpy()
            V = torch.cat([c.v[st:st + n], c.v_new[h, vis[p]]]).double().numpy()
            if c.kind == "uniform":
                x = np.zeros((G, K.shape[0]))
            else:
                x = c.q[h, p].double().numpy() @ K.T
                assert np.array_equal(x, np.round(x))
            P = np.exp2(x - x.max(-1, keepdims=True))
            num[h, p], den[h, p] = P @ V, P.sum(-1)
    return ap.finalize(num, den, c.dtype, "div")


def concat_for_oracle(c: sp.SpecCase, parents: List[int], p: int):
    """What node p sees as one flat ragged cache - per head the old rows with the rows of p's ancestors and its own behind them:
    (k, v [rows, D], starts, lens) for ``orc.varlen_attn`` with q_len = 1."""
    vis = visible(parents)[p]
    ks, vs, starts, lens, acc = [], [], [], [], 0
    for h in range(len(c.lens)):
        st, n = c.starts[h], c.lens[h]
        ks += [c.k[st:st + n], c.k_new[h, vis]]
        vs += [c.v[st:st + n], c.v_new[h, vis]]
        starts.append(acc); lens.append(n + len(vis)); acc += n + len(vis)
    return torch.cat(ks), torch.cat(vs), starts, lens
