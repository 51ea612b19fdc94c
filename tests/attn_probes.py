"""Attention probes whose correct 16-bit output is known EXACTLY (host-only helpers of the exact attention tests).

Random inputs leave an attention kernel an error budget (1e-3 absolute) that one key counted wrongly stays inside at decode
magnitudes.  These inputs are chosen so that every weight, every partial sum and every merge of a correct kernel is exact in fp32;
what is left is the kernel's final normalisation and its 16-bit cast, which are emulated here bit for bit.  A GPU test can then
compare bits.

* Uniform probe: q = 0, so every visible logit is 0 and every p = exp2(0) = 1 (also after P is rounded to 16 bits); l is the
  number of visible keys.  V rows are 0/1 vectors that mark keys: dense marking (key j sets dim j mod D) where a head is short
  enough for one key to move an output by several 16-bit steps, sparse marking (only the boundary keys, each on its own dim
  round-robin) on long heads.  Slack rows after a segment hold a large value, so a key read past its segment is visible too.
* Weighted probe: softmax_scale = SCALE_ONE, for which fp32(scale * log2e) == 1.0f (the fold every kernel does first), q one-hot
  per query row, so a logit is one integer entry of K.  Entries lie in [-spread, 0] with one 0 (the row's maximum) per dim at a
  random key: every weight is a power of two and every partial and combined sum is exact in fp32 while
  spread + log2(n) (+ F2_DEFER for the 32-row kernel's deferred rescale) <= 24.

Final normalisation (checked in the code; the library is built without fast-math, so fp32 division - also 1 / l - is the
correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence):
  * decode combine (kvz_attn.hip):            out = fp16/bf16(a / l)
  * kvz_flash, kvz_flash2 and their combines: out = fp16/bf16(a * fp32(1 / l))
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

LOG2E_F32 = np.float32(1.44269504088896340736)
SCALE_ONE = float(np.float32(np.float32(1.0) / LOG2E_F32))     # 0.6931472f: fp32(SCALE_ONE * log2e) == 1.0f exactly
assert np.float32(SCALE_ONE) * LOG2E_F32 == np.float32(1.0)
F2_DEFER = 6            # kvz_flash2.hip: exp2-domain slack of the deferred rescale (P <= 2^6)
SLACK_VALUE = 64.0      # V (and K) of the slack rows behind a segment: a key read past its segment moves the output visibly


def decode_chunk(lens: Sequence[int], items: int) -> int:
    """Keys per work item of the decode kernel (kvz_attn.hip): cut from the SUM of the head lengths, a multiple of 128."""
    total = sum(lens)
    chunk = (total + items - 1) // items
    chunk = (chunk + 127) // 128 * 128
    return max(chunk, 128)


def decode_edges(n: int, chunk: int) -> List[int]:
    """First and last key of every split of a head of n keys."""
    out = []
    for c0 in range(0, n, chunk):
        out += [c0, min(n, c0 + chunk) - 1]
    return out


@dataclass
class Probe:
    q: torch.Tensor               # [Hkv*q_len, G, D] 16-bit (CPU)
    k: torch.Tensor               # [rows, D]
    v: torch.Tensor               # [rows, D]
    starts: List[int]
    lens: List[int]               # keys of every head the probe holds rows for (the attention call may see fewer)
    q_len: int
    causal: bool
    scale: float
    kind: str
    marks: Dict[int, List[int]] = field(default_factory=dict)   # head -> marked keys (uniform probe)

    @property
    def dtype(self):
        return self.q.dtype


def _layout(lens, slack):
    starts, acc = [], 0
    for n in lens:
        starts.append(acc)
        acc += n + slack
    return starts, max(acc, 1)


def boundary_keys(n: int, q_len: int, all_lens: Sequence[int], items: Sequence[int]) -> List[int]:
    """Keys of a head of n keys where kernels cut: segment ends, causal limits, split edges of every `items` value, tile edges
    of the first and last 256 keys (16/32/64-key tiles)."""
    if n == 0:
        return []
    ks = {0, n - 1}
    ks.update(range(max(0, n - q_len - 1), n))
    for it in items:
        ks.update(decode_edges(n, decode_chunk(all_lens, it)))
    for t in range(0, min(n, 256), 16):
        ks.update((t, t - 1))
    last = (n - 1) // 16 * 16
    for t in range(max(0, last - 256), n + 1, 16):
        ks.update((t, t - 1))
    return sorted(x for x in ks if 0 <= x < n)


def uniform_probe(lens: Sequence[int], q_len: int, G: int, D: int, dtype, causal: bool = True, items: Sequence[int] = (),
                  slack: int = 3, seed: int = 0, dense_max: Optional[int] = None, marks_lens: Optional[Sequence[int]] = None) -> Probe:
    """q = 0; V marks keys.  `items`: the attn_items values whose split edges a sparsely marked head marks; `marks_lens`: the head
    lengths the decode kernel will see (default `lens`), from which those edges are computed."""
    lens = [int(n) for n in lens]
    g = torch.Generator().manual_seed(seed)
    starts, rows = _layout(lens, slack)
    Hkv = len(lens)
    dense_max = 16 * D if dense_max is None else dense_max
    k = torch.randn(rows, D, generator=g)
    v = torch.full((rows, D), SLACK_VALUE)
    marks = {}
    ml = list(lens if marks_lens is None else marks_lens)
    for h, n in enumerate(lens):
        st = starts[h]
        v[st:st + n] = 0
        if n <= dense_max:
            keys = list(range(n))
            v[st + torch.arange(n), torch.arange(n) % D] = 1
        else:
            keys = boundary_keys(n, q_len, ml, items)
            for i, j in enumerate(keys):
                v[st + j, i % D] = 1
        marks[h] = keys
    q = torch.zeros(Hkv * q_len, G, D)
    return Probe(q.to(dtype), k.to(dtype), v.to(dtype), starts, lens, q_len, causal, 1.0 / math.sqrt(D), "uniform", marks)


def weighted_probe(lens: Sequence[int], q_len: int, G: int, D: int, dtype, causal: bool = True, spread: int = 8, slack: int = 3,
                   seed: int = 0, headroom: int = 0) -> Probe:
    """q one-hot per query row (row r of head h selects dim (r + 5h) mod D), K integer in [-spread, -1] with one 0 per dim at a
    random key, V random 0/1.  `headroom`: exponent bits a kernel may need beyond spread + log2(n) (F2_DEFER for kvz_flash2)."""
    lens = [int(n) for n in lens]
    for n in lens:
        assert spread + math.ceil(math.log2(n + 1)) + headroom <= 24, ("fp32 sums would round", n, spread, headroom)
    g = torch.Generator().manual_seed(seed)
    starts, rows = _layout(lens, slack)
    Hkv = len(lens)
    k = torch.full((rows, D), SLACK_VALUE)
    v = torch.full((rows, D), SLACK_VALUE)
    for h, n in enumerate(lens):
        st = starts[h]
        if n == 0:
            continue
        k[st:st + n] = -torch.randint(1, spread + 1, (n, D), generator=g).float()
        k[st + torch.randint(0, n, (D,), generator=g), torch.arange(D)] = 0.0
        v[st:st + n] = torch.randint(0, 2, (n, D), generator=g).float()
    R = q_len * G
    q = torch.zeros(Hkv, R, D)
    r = torch.arange(R)
    for h in range(Hkv):
        q[h, r, (r + 5 * h) % D] = 1.0
    q = q.view(Hkv * q_len, G, D)
    return Probe(q.to(dtype), k.to(dtype), v.to(dtype), starts, lens, q_len, causal, SCALE_ONE, "weighted", {})


# ---- exact expectation -------------------------------------------------------------------------------------------------------
def head_weights(p: Probe, h: int, n: int, limit_shift: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(P [q_len*G, n] float64 exact powers of two, 0 where invisible; V [n, D] float64) of head h over its first n keys."""
    D = p.q.shape[-1]
    G = p.q.shape[1]
    st = p.starts[h]
    K = p.k[st:st + n].double().numpy()
    V = p.v[st:st + n].double().numpy()
    Q = p.q[h * p.q_len:(h + 1) * p.q_len].double().numpy().reshape(p.q_len * G, D)
    if p.kind == "uniform":
        x = np.zeros((p.q_len * G, n))
    else:
        x = Q @ K.T                                    # integer logits in the exp2 domain (scale folds to 1.0)
        assert np.array_equal(x, np.round(x))
    i = np.arange(p.q_len * G) // G
    j = np.arange(n)
    vis = (j[None, :] <= (i[:, None] + n - p.q_len + limit_shift)) if p.causal else np.ones((p.q_len * G, n), bool)
    x = np.where(vis, x, -np.inf)
    M = x.max(-1, keepdims=True) if n else np.full((p.q_len * G, 1), -np.inf)
    M = np.where(np.isinf(M), 0.0, M)
    P = np.where(vis, np.exp2(x - M), 0.0)
    return P, V, M[:, 0]


def exact_num_den(p: Probe, lens: Optional[Sequence[int]] = None, limit_shift: int = 0):
    """Exact numerator [Hkv*q_len, G, D], denominator [Hkv*q_len, G] and row maximum (exp2 domain) of the softmax-weighted sum, for
    the head lengths `lens` the call sees (default: the probe's)."""
    lens = p.lens if lens is None else list(lens)
    HQ, G, D = p.q.shape
    num = np.zeros((HQ, G, D))
    den = np.zeros((HQ, G))
    mx = np.zeros((HQ, G))
    for h, n in enumerate(lens):
        P, V, M = head_weights(p, h, n, limit_shift)
        sl = slice(h * p.q_len, (h + 1) * p.q_len)
        num[sl] = (P @ V).reshape(p.q_len, G, D)
        den[sl] = P.sum(-1).reshape(p.q_len, G)
        mx[sl] = M.reshape(p.q_len, G)
    return num, den, mx


def finalize(num: np.ndarray, den: np.ndarray, dtype, norm: str) -> torch.Tensor:
    """The kernel's last two roundings: fp32 a / l (norm 'div') or a * fp32(1 / l) ('rcp'), then RNE to the 16-bit dtype.  The sums
    themselves must be exact in fp32 (asserted)."""
    a = num.astype(np.float32)
    l = den.astype(np.float32)
    assert np.array_equal(a.astype(np.float64), num) and np.array_equal(l.astype(np.float64), den), "probe sums not exact in fp32"
    with np.errstate(divide="ignore", invalid="ignore"):
        if norm == "div":
            o = np.where(l[..., None] > 0, a / l[..., None], np.float32(0))
        elif norm == "rcp":
            r = np.where(l > 0, np.float32(1) / l, np.float32(0)).astype(np.float32)
            o = a * r[..., None]
        else:
            raise ValueError(norm)
    return torch.from_numpy(o.astype(np.float32)).to(dtype)


def expected(p: Probe, norm: str, lens: Optional[Sequence[int]] = None) -> torch.Tensor:
    num, den, _ = exact_num_den(p, lens)
    return finalize(num, den, p.dtype, norm)


def expected_lse(p: Probe, lens: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """fp64 natural-log LSE [Hkv*q_len, G] of the exact sums, (M + log2 l) * ln 2 (-inf for rows without a key), and the magnitude
    |M| + log2 l of the fp32 sum the kernels form BEFORE the scaling by ln 2 (M + log2f(l): half an ulp of that sum for the add, about
    one for log2f, half an ulp of the result for the product), at which their ulps are counted."""
    _, den, mx = exact_num_den(p, lens)
    with np.errstate(divide="ignore"):
        lse = np.where(den > 0, (mx + np.log2(den)) * math.log(2.0), -np.inf)
        mag = np.where(den > 0, np.abs(mx) + np.log2(np.maximum(den, 1)), 0.0)
    return lse, mag


def bits_equal(got: torch.Tensor, want: torch.Tensor) -> Tuple[bool, int]:
    """(bit-identical?, number of differing elements) of two 16-bit tensors."""
    a = got.detach().cpu().contiguous().view(torch.int16)
    b = want.detach().cpu().contiguous().view(torch.int16)
    d = int((a != b).sum())
    return d == 0, d


def steps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|a - b| in 16-bit grid steps (monotone integer order of the bit patterns)."""
    def key(t):
        x = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
        return torch.where(x >= 0x8000, 0x8000 - (x - 0x8000) - 1, x + 0x8000)
    return (key(a) - key(b)).abs()


# ---- injected faults (CPU only): how far one key counted wrongly moves the expectation ------------------------------------------
def key_fault_steps(p: Probe, norm: str, lens: Optional[Sequence[int]] = None):
    """For every marked key of every head and every query row that sees it: the 16-bit steps (and the absolute change) by which
    the expected output moves on the key's own dims when the key is dropped, and when it is counted twice (rows where it is the
    only visible key excepted: doubling a sole key is invisible to any input).
    Returns {"drop": (min_steps, min_abs, max_abs, cases), "dup": (...)} over all (key, row) pairs (kinds without a case left out)."""
    lens = p.lens if lens is None else list(lens)
    res = {"drop": [10 ** 9, math.inf, 0.0, 0], "dup": [10 ** 9, math.inf, 0.0, 0]}
    for h, n in enumerate(lens):
        keys = [j for j in p.marks.get(h, []) if j < n]
        if not keys:
            continue
        P, V, _ = head_weights(p, h, n)
        num = P @ V
        den = P.sum(-1)
        base = finalize(num, den, p.dtype, norm)
        J = np.array(keys)
        for kind, sgn in (("drop", -1.0), ("dup", 1.0)):
            for d in range(V.shape[1]):
                jd = J[V[J, d] == 1]
                if jd.size == 0:
                    continue
                pj = P[:, jd]                                     # [R, m]
                seen = pj > 0
                if kind == "dup":   # (a row's only visible key counted twice leaves every softmax unchanged: no input can see it)
                    seen &= pj < den[:, None]
                n2 = num[:, d:d + 1] + sgn * pj
                d2 = den[:, None] + sgn * pj
                # every other dim keeps its numerator: the marked dim is the one that must move
                fo = finalize(n2[..., None], d2, p.dtype, norm)[..., 0]
                b = base[:, d:d + 1].expand_as(fo)
                sel = torch.from_numpy(seen)
                s = steps(fo, b)[sel]
                if s.numel():
                    a = (fo.float() - b.float()).abs()[sel]
                    r = res[kind]
                    r[0], r[1], r[2] = min(r[0], int(s.min())), min(r[1], float(a.min())), max(r[2], float(a.max()))
                    r[3] += int(s.numel())
    return {k: tuple(v) for k, v in res.items() if v[3]}


def causal_fault_steps(p: Probe, norm: str, lens: Optional[Sequence[int]] = None):
    """The causal limit of every query row moved by -1 and by +1: per shift, the smallest number of 16-bit steps by which a row
    whose visible set changes moves (its largest element change), the smallest and largest absolute change of such a row, and the
    number of rows."""
    lens = p.lens if lens is None else list(lens)
    base = expected(p, norm, lens)
    HQ, G, D = p.q.shape
    out = {}
    for shift in (-1, 1):
        num, den, _ = exact_num_den(p, lens, limit_shift=shift)
        f = finalize(num, den, p.dtype, norm)
        changed = torch.zeros(HQ, G, dtype=torch.bool)
        for h, n in enumerate(lens):
            i = torch.arange(p.q_len)
            lim = i + n - p.q_len
            moved = ((lim + shift).clamp(-1, n - 1) != lim.clamp(-1, n - 1))
            changed[h * p.q_len:(h + 1) * p.q_len] = moved[:, None].expand(p.q_len, G)
        if not bool(changed.any()):
            continue
        s = steps(f, base).amax(-1)[changed]
        a = (f.float() - base.float()).abs().amax(-1)[changed]
        out[shift] = (int(s.min()), float(a.min()), float(a.max()), int(changed.sum()))
    return out
