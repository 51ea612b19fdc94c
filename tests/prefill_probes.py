"""Packed-first-step probes whose correct 16-bit output is known EXACTLY (host-only helpers; the method of tests/attn_probes.py and
tests/fork_probes.py).

A case is one call of ``kvz_fork_prefill_tail``: B branches, their queries back to back (branch b owns packed positions
``cu_q[b] : cu_q[b + 1]``, possibly none), per-branch tails, the new K,V rows of all positions, and a partial result over the shared
segments ``(o_shared, lse_shared)``.  With ``lse_shared = -inf`` everywhere the result is the tail attention alone.

* Uniform probe: q = 0, every visible key weighs 1.  V marks keys on DISTINCT dims: key j of a branch (old tail rows first, then its
  new rows) on dim j mod (D - 3), old tail rows on dim D - 3, new rows on dim D - 2, and dim D - 1 of every row holds the branch
  number b + 1 - so a key too many or too few, or a row of another branch, moves an output by whole 16-bit steps, and dim D - 1 of
  every output row of branch b is exactly b + 1.  Unused tail rows hold ``SLACK_VALUE``.
* Weighted probe: ``SCALE_ONE``, one-hot q (packed position i, group member g of head h selects dim (i*G + g + 5h) mod D), integer K
  in [-spread, 0], V in {0, 1}: every weight is a power of two and every sum is exact in fp32.
* Merge: ``o_shared`` holds multiples of 1/8 and ``lse_shared`` holds +-2^j * ``SCALE_ONE`` (or -inf), whose product with fp32 log2(e)
  is exactly +-2^j: both weights of the merge are powers of two.

The kernel's last roundings (kvz_fork_prefill.hip): out = fp16/bf16((w1 * o_shared + w2 * a) / (w1 + w2 * l)) - one fp32 division of
two exact sums, one cast.  ``expected_out`` also evaluates the quotient in float64 and asserts that its cast gives the same bits.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

import attn_probes as ap

NEG_INF = float("-inf")


@dataclass
class PrefillCase:
    q: torch.Tensor            # [Hkv, T, G, D]
    cu_q: List[int]            # B + 1
    tail_k: torch.Tensor       # [B, Hkv, cap, D]
    tail_v: torch.Tensor
    tail_len: List[int]
    k_new: torch.Tensor        # [Hkv, T, D]
    v_new: torch.Tensor
    o_shared: torch.Tensor     # [Hkv, T, G, D]
    lse_shared: torch.Tensor   # [Hkv, T, G] fp32
    scale: float
    kind: str

    @property
    def dtype(self):
        return self.q.dtype

    @property
    def lengths(self):
        return [self.cu_q[b + 1] - self.cu_q[b] for b in range(len(self.tail_len))]


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + int(n))
    return cu


def _no_shared(Hkv, T, G, D, dtype):
    """A shared side that saw no key: lse -inf, and NaN where its output would be (a weight of 0 silences whatever is there)."""
    return torch.full((Hkv, T, G, D), float("nan")).to(dtype), torch.full((Hkv, T, G), NEG_INF, dtype=torch.float32)


def uniform_case(lengths: Sequence[int], tail_len: Sequence[int], G: int, D: int, dtype, tail_cap: int, Hkv: int = 2,
                 seed: int = 0) -> PrefillCase:
    B, cu = len(lengths), _cu(lengths)
    T = cu[-1]
    assert len(tail_len) == B and all(t + n <= tail_cap for t, n in zip(tail_len, lengths))
    g = torch.Generator().manual_seed(seed)
    tk = torch.full((B, Hkv, tail_cap, D), ap.SLACK_VALUE)
    tv = torch.full((B, Hkv, tail_cap, D), ap.SLACK_VALUE)
    k_new = torch.randn(Hkv, T, D, generator=g)
    v_new = torch.zeros(Hkv, T, D)
    for b in range(B):
        t, n = tail_len[b], lengths[b]
        rows = torch.zeros(t + n, D)
        j = torch.arange(t + n)
        rows[j, j % (D - 3)] = 1
        rows[:t, D - 3] = 1
        rows[t:, D - 2] = 1
        rows[:, D - 1] = b + 1
        tk[b, :, :t] = torch.randn(Hkv, t, D, generator=g)
        tv[b, :, :t] = rows[:t]
        v_new[:, cu[b]:cu[b + 1]] = rows[t:]
    o, lse = _no_shared(Hkv, T, G, D, dtype)
    return PrefillCase(torch.zeros(Hkv, T, G, D).to(dtype), cu, tk.to(dtype), tv.to(dtype), list(tail_len), k_new.to(dtype),
                       v_new.to(dtype), o, lse, 1.0 / D ** 0.5, "uniform")


def weighted_case(lengths: Sequence[int], tail_len: Sequence[int], G: int, D: int, dtype, tail_cap: int, Hkv: int = 2,
                  spread: int = 8, seed: int = 0) -> PrefillCase:
    B, cu = len(lengths), _cu(lengths)
    T = cu[-1]
    assert len(tail_len) == B and all(t + n <= tail_cap for t, n in zip(tail_len, lengths))
    g = torch.Generator().manual_seed(seed)
    tk = torch.full((B, Hkv, tail_cap, D), ap.SLACK_VALUE)
    tv = torch.full((B, Hkv, tail_cap, D), ap.SLACK_VALUE)
    for b, t in enumerate(tail_len):
        tk[b, :, :t] = -torch.randint(0, spread + 1, (Hkv, t, D), generator=g).float()
        tv[b, :, :t] = torch.randint(0, 2, (Hkv, t, D), generator=g).float()
    k_new = -torch.randint(0, spread + 1, (Hkv, T, D), generator=g).float()
    v_new = torch.randint(0, 2, (Hkv, T, D), generator=g).float()
    q = torch.zeros(Hkv, T, G, D)
    for h in range(Hkv):
        r = torch.arange(T * G)
        q[h].view(T * G, D)[r, (r + 5 * h) % D] = 1.0
    o, lse = _no_shared(Hkv, T, G, D, dtype)
    return PrefillCase(q.to(dtype), cu, tk.to(dtype), tv.to(dtype), list(tail_len), k_new.to(dtype), v_new.to(dtype), o, lse,
                       ap.SCALE_ONE, "weighted")


def with_shared(c: PrefillCase, seed: int = 0) -> PrefillCase:
    """The same case with a shared side: o_shared multiples of 1/8 in [-2, 2], lse_shared in {-inf, +-SCALE_ONE * 2^j}."""
    Hkv, T, G, D = c.q.shape
    g = torch.Generator().manual_seed(seed + 17)
    o = (torch.randint(-16, 17, (Hkv, T, G, D), generator=g).float() / 8).to(c.dtype)
    exps = torch.tensor([NEG_INF, -4.0, -2.0, -1.0, 1.0, 2.0, 4.0])
    lse = (exps[torch.randint(0, len(exps), (Hkv, T, G), generator=g)] * np.float32(ap.SCALE_ONE)).float()
    return PrefillCase(c.q, c.cu_q, c.tail_k, c.tail_v, c.tail_len, c.k_new, c.v_new, o, lse, c.scale, c.kind)


def row_keys(c: PrefillCase, b: int, h: int, p: int, fault: Optional[str] = None):
    """(K, V) float64 [n, D] that packed position cu_q[b] + p of branch b sees at head h: tail rows 0 .. t_b - 1 ++ its branch's new
    rows 0 .. p.  ``fault`` plays a wrong kernel: 'key+1' lets the row see the next new row as well (where the branch has one),
    'foreign' adds the first new row of the next branch that has any."""
    t, c0 = c.tail_len[b], c.cu_q[b]
    hi = p + 1
    if fault == "key+1":
        hi = min(p + 2, c.cu_q[b + 1] - c0)
    ks, vs = [c.tail_k[b, h, :t], c.k_new[h, c0:c0 + hi]], [c.tail_v[b, h, :t], c.v_new[h, c0:c0 + hi]]
    if fault == "foreign":
        B = len(c.tail_len)
        other = next(o for o in ((b + 1 + i) % B for i in range(B)) if o != b and c.cu_q[o + 1] > c.cu_q[o])
        ks.append(c.k_new[h, c.cu_q[other]:c.cu_q[other] + 1])
        vs.append(c.v_new[h, c.cu_q[other]:c.cu_q[other] + 1])
    return torch.cat(ks).double().numpy(), torch.cat(vs).double().numpy()


def expected_out(c: PrefillCase, fault: Optional[str] = None) -> torch.Tensor:
    """[Hkv, T, G, D] in the case's dtype: the exact sums of the merge, the kernel's one division and one cast."""
    Hkv, T, G, D = c.q.shape
    num = np.zeros((Hkv, T, G, D))
    den = np.zeros((Hkv, T, G))
    x1 = c.lse_shared.numpy().astype(np.float32) * ap.LOG2E_F32            # the kernel's fp32 product: exactly +-2^j or -inf
    assert np.array_equal(x1[np.isfinite(x1)], np.round(x1[np.isfinite(x1)])), "lse_shared * log2(e) must be an integer in fp32"
    x1 = x1.astype(np.float64)
    o1 = np.where(np.isfinite(x1)[..., None], c.o_shared.double().numpy(), 0.0)
    for b in range(len(c.tail_len)):
        for p in range(c.cu_q[b + 1] - c.cu_q[b]):
            i = c.cu_q[b] + p
            for h in range(Hkv):
                K, V = row_keys(c, b, h, p, fault)
                if c.kind == "uniform":
                    x = np.zeros((G, K.shape[0]))
                else:
                    x = c.q[h, i].double().numpy() @ K.T
                    assert np.array_equal(x, np.round(x))
                m = x.max(-1)
                P = np.exp2(x - m[:, None])
                M = np.maximum(x1[h, i], m)
                w1, w2 = np.exp2(x1[h, i] - M), np.exp2(m - M)
                num[h, i] = w1[:, None] * o1[h, i] + w2[:, None] * (P @ V)
                den[h, i] = w1 + w2 * P.sum(-1)
    out = ap.finalize(num, den, c.dtype, "div")
    once = torch.from_numpy(num / den[..., None]).to(c.dtype)               # float64 quotient, cast once
    assert ap.bits_equal(out, once)[0], "the fp32 division and the float64 quotient round to different 16-bit values"
    return out


def expected_tails(c: PrefillCase):
    """(tail_k, tail_v) after the call: rows t_b .. t_b + n_b - 1 hold the branch's new rows, every other byte as before."""
    tk, tv = c.tail_k.clone(), c.tail_v.clone()
    for b, t in enumerate(c.tail_len):
        n = c.cu_q[b + 1] - c.cu_q[b]
        tk[b, :, t:t + n], tv[b, :, t:t + n] = c.k_new[:, c.cu_q[b]:c.cu_q[b + 1]], c.v_new[:, c.cu_q[b]:c.cu_q[b + 1]]
    return tk, tv


def as_model_tensors(c: PrefillCase):
    """(query [1, H, T, D], k_new, v_new [1, Hkv, T, D]) as the attention layer hands them over: transposed views of [1, T, heads, D]."""
    Hkv, T, G, D = c.q.shape
    q = c.q.permute(1, 0, 2, 3).reshape(1, T, Hkv * G, D).transpose(1, 2)
    k = c.k_new.transpose(0, 1).reshape(1, T, Hkv, D).contiguous().transpose(1, 2)
    v = c.v_new.transpose(0, 1).reshape(1, T, Hkv, D).contiguous().transpose(1, 2)
    return q, k, v
