"""Selection probes: score tensors built from 16-bit PATTERNS with declared multiplicities, for the five entry points of the selection
stage (kvz_select_threshold, kvz_select_threshold_prehist fed by kvz_score_finalize_log_hist, kvz_select_topk_rows, kvz_select_heads,
kvz_rowmax16).  Host only: numpy + torch on the CPU.

The random-score tests draw rand() ** k: non-negative, finite, smooth over the radix bins.  These probes hold what those never do - NaNs
of both signs and every payload, infinities, subnormals, both zeros, multisets inside one 11-bit bin, ranks on bin edges - and put
them where the kernels change code path (the last n % 8 elements: block 0's tail loop; row starts; rows with row_len % 8 != 0: the
scalar emit).

What a probe expects follows by COUNTING over value classes, not by sorting: the reference (attention/score.py:88-120) orders scores
as numbers, with every NaN above +inf (torch.sort / torch.topk) and +0 == -0, so the value class of a pattern is

    class_key = 0xFFFF for a NaN (either sign, any payload), 0x8000 for +0 and -0, else the monotone 16-bit order key

and the threshold of rank idx is the class t with  #(class > t) <= idx < #(class >= t);  the mask is class > t without the NaNs
(score > thres compares floats: a NaN takes a rank but is never kept, and a NaN threshold keeps nothing).  Per-row top-k, which
scatters indices, keeps every class > t - NaNs included - and the lowest-index entries of class t.

`radix_threshold` / `radix_topk` restate the kernels' two-level 11 + 5 bit radix selection and ordered tie emit in numpy with the key,
the compare and the rank pluggable.  They audit the probes (tests/test_select_probes.py: each fault injected there must change what
some probe expects); they are not a second oracle."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
INF = {F16: 0x7C00, BF16: 0x7F80}          # +inf; a pattern is a NaN when its magnitude bits exceed this
NAN_CLASS, ZERO_CLASS = 0xFFFF, 0x8000


def tag(dtype) -> str:
    return "f16" if dtype == F16 else "bf16"


def to_tensor(bits: np.ndarray, dtype) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(dtype)


def to_f32(bits: np.ndarray, dtype) -> np.ndarray:
    return to_tensor(bits, dtype).float().numpy()


def is_nan(bits, dtype):
    return (np.asarray(bits, dtype=np.uint32) & 0x7FFF) > INF[dtype]


# ---- keys --------------------------------------------------------------------------------------------------------------------------
def order_key(bits, dtype):
    """the kernels' key (kvz_common.h order_key16): monotone in the value, every NaN above +inf whatever its sign (the sign of a NaN
    is dropped, its payload kept), -0 one step below +0"""
    b = np.asarray(bits, dtype=np.uint32)
    neg = ((b & 0x8000) != 0) & ((b & 0x7FFF) <= INF[dtype])
    return np.where(neg, ~b & 0xFFFF, b | 0x8000).astype(np.uint32)


def order_key_sign_only(bits, dtype):
    """the key before NaNs were given a place: a sign-bit NaN sorts below -inf"""
    b = np.asarray(bits, dtype=np.uint32)
    return np.where((b & 0x8000) != 0, ~b & 0xFFFF, b | 0x8000).astype(np.uint32)


def class_key(bits, dtype):
    """value class: NaN == NaN, +0 == -0 (the key of the per-row top-k, kvz_common.h class_key16)"""
    b = np.asarray(bits, dtype=np.uint32)
    k = order_key(b, dtype)
    k = np.where((b & 0x7FFF) > INF[dtype], NAN_CLASS, k)
    return np.where((b & 0x7FFF) == 0, ZERO_CLASS, k).astype(np.uint32)


def key_inv(key):
    k = np.asarray(key, dtype=np.uint32)
    return np.where((k & 0x8000) != 0, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint16)


def same_class(a_bits, b_bits, dtype) -> bool:
    """two thresholds are the same number: equal bits, both NaN, or both zero (which NaN payload / which zero the reference's sort
    leaves at the rank is its unspecified order among equal values; the mask does not depend on it)"""
    return int(class_key(a_bits, dtype)) == int(class_key(b_bits, dtype))


def f32_to_bits(x: float, dtype) -> int:
    """a threshold returned as a float -> its 16-bit pattern (exact: thresholds ARE 16-bit values)"""
    t = torch.tensor([x], dtype=torch.float32).to(dtype)
    return int(t.view(torch.int16).item()) & 0xFFFF


# ---- expectation by counting ------------------------------------------------------------------------------------------------------------
def rank_of_ratio(n: int, ratio: float) -> int:
    return max(int(n * ratio) - 1, 0)          # attention/score.py:95


def ratio_for_rank(n: int, idx: int) -> float:
    """a ratio < 1 with rank_of_ratio(n, ratio) == idx (0 <= idx <= n - 2)"""
    assert 0 <= idx <= n - 2, (n, idx)
    r = (idx + 1.5) / n
    assert r < 1 and rank_of_ratio(n, r) == idx, (n, idx, r)
    return r


def class_at_rank(keys: np.ndarray, idx: int) -> Tuple[int, int]:
    """(class t, number of entries of a class above t) with  #(> t) <= idx < #(>= t)"""
    cnt = np.bincount(keys.reshape(-1), minlength=65536)
    at_least = cnt[::-1].cumsum()                    # at_least[j] = #(key >= 65535 - j)
    j = int(np.searchsorted(at_least, idx, side="right"))
    t = 65535 - j
    return t, int(at_least[j] - cnt[t])


@dataclass
class Expect:
    thres_bits: int            # canonical pattern of the threshold's class (0x7FFF: NaN, 0: zero); compare with same_class
    valid: np.ndarray          # bool, shape of the probe
    kept: int
    row_counts: np.ndarray     # int32 per row


def expect_threshold(bits: np.ndarray, ratio: float, dtype) -> Expect:
    rows = bits.reshape(-1, bits.shape[-1])
    if not ratio < 1:
        v = np.ones(bits.shape, dtype=bool)
        return Expect(0, v, v.size, np.full(rows.shape[0], rows.shape[1], np.int32))
    ck = class_key(bits, dtype)
    t, _ = class_at_rank(ck, rank_of_ratio(bits.size, ratio))
    v = (ck > t) & (ck != NAN_CLASS)                 # (score > thres as floats: a NaN takes a rank but is never kept)
    return Expect(int(key_inv(t)), v, int(v.sum()), v.reshape(rows.shape).sum(-1).astype(np.int32))


def expect_heads(bits: np.ndarray, n_ctx: int, ratio: float, dtype) -> Expect:
    """head-level selection: every head value stands n_ctx times in the expanded tensor the reference sorts (model/wrapper.py:54-57)"""
    if not ratio < 1:
        v = np.ones(bits.shape, dtype=bool)
        return Expect(0, v, v.size * n_ctx, np.full(bits.size, n_ctx, np.int32))
    ck = class_key(bits, dtype)
    t, _ = class_at_rank(ck, rank_of_ratio(bits.size * n_ctx, ratio) // n_ctx)
    v = (ck > t) & (ck != NAN_CLASS)
    return Expect(int(key_inv(t)), v, int(v.sum()) * n_ctx, (v.reshape(-1) * n_ctx).astype(np.int32))


def expect_topk(bits: np.ndarray, k: int, dtype) -> np.ndarray:
    """per row: every class above the k-th largest, then the lowest-index entries of that class until k are kept"""
    rows = bits.reshape(-1, bits.shape[-1])
    out = np.zeros(rows.shape, dtype=bool)
    if k <= 0:
        return out.reshape(bits.shape)
    if k >= rows.shape[1]:
        return np.ones(bits.shape, dtype=bool)
    ck = class_key(rows, dtype)
    for r in range(rows.shape[0]):
        t, above = class_at_rank(ck[r], k - 1)
        tie = ck[r] == t
        out[r] = (ck[r] > t) | (tie & (np.cumsum(tie) <= k - above))
    return out.reshape(bits.shape)


def check_topk_contract(case: str, bits: np.ndarray, valid: np.ndarray, ref_valid: np.ndarray, k: int, dtype) -> int:
    """conftest.check_uniform_contract restated on value classes, so that it holds for rows with NaNs too (there `s != kth` is true
    everywhere and torch.equal of two tensors with a NaN is false): exactly k per row, the same multiset of kept classes, the
    identical mask wherever a score's class differs from the row's boundary class.  Returns the entries placed differently."""
    rows = bits.reshape(-1, bits.shape[-1])
    v, r = valid.reshape(rows.shape).astype(bool), ref_valid.reshape(rows.shape).astype(bool)
    assert (v.sum(-1) == k).all() and (r.sum(-1) == k).all(), (case, "kept per row != k")
    ck = class_key(rows, dtype).astype(np.int64)
    for i in range(rows.shape[0]):
        t, _ = class_at_rank(ck[i], k - 1)
        off = ck[i] != t
        assert np.array_equal(v[i] & off, r[i] & off), (case, i, "mask differs away from the boundary class")
        assert np.array_equal(np.sort(ck[i][v[i]]), np.sort(ck[i][r[i]])), (case, i, "kept multiset differs")
    return int((v != r).sum())


# ---- the reference's expressions, evaluated by torch on the CPU --------------------------------------------------------------------------
def ref_threshold(score: torch.Tensor, ratio: float):
    """attention/score.py:93-100 restated line by line"""
    if ratio < 1:
        score_sort = torch.sort(score.reshape(-1), descending=True).values
        n = max(int(len(score_sort) * ratio) - 1, 0)
        thres = score_sort[n].item()
        return torch.where(score > thres, True, False).bool(), thres
    return torch.ones_like(score, dtype=bool), 0.


def ref_topk(score: torch.Tensor, k: int) -> torch.Tensor:
    """attention/score.py:112-114"""
    _, idx = torch.topk(score, k, dim=-1)
    valid = torch.zeros_like(score, dtype=bool)
    valid.scatter_(-1, idx, True)
    return valid


# ---- numpy restatement of the kernels (pluggable key / compare / rank): audits the probes ------------------------------------------------
def _find_desc(hist: np.ndarray, idx: int, ascending: bool = False):
    """(bin, residual rank) of a descending cumulative search, None when idx lies beyond the total"""
    order = range(len(hist)) if ascending else range(len(hist) - 1, -1, -1)
    above = 0
    for b in order:
        if above <= idx < above + int(hist[b]):
            return b, idx - above
        above += int(hist[b])
    return None


def radix_threshold(bits: np.ndarray, ratio: float, dtype, key: Callable = order_key, rank_off: int = 0, emit: str = "gt",
                    skip_tail: Optional[str] = None, lo_ascending: bool = False) -> Tuple[int, np.ndarray]:
    """kvz_select_threshold: histogram of the top 11 key bits, of the low 5 bits inside the bin that holds the rank, then
    valid = value > threshold as FLOATS.  -> (threshold bits, mask).  Faults: `key`, `rank_off`, emit "ge" / "key" (compare keys:
    keeps NaNs), skip_tail "hi" / "lo" (the last n % 8 elements missing from that histogram), lo_ascending."""
    flat = bits.reshape(-1)
    n = flat.size
    if not ratio < 1:
        return 0, np.ones(bits.shape, dtype=bool)
    idx = min(max(rank_of_ratio(n, ratio) + rank_off, 0), n - 1)
    keys = key(flat, dtype)
    body = n - (n % 8)
    hi = keys >> 5
    found = _find_desc(np.bincount(hi[:body] if skip_tail == "hi" else hi, minlength=2048), idx)
    if found is not None:
        b, rank = found
        sel = keys[:body] if skip_tail == "lo" else keys
        found = _find_desc(np.bincount(sel[(sel >> 5) == b] & 31, minlength=32), rank, ascending=lo_ascending)
    if found is None:                                  # the histograms do not hold the rank: NaN threshold, nothing kept
        return 0x7FFF, np.zeros(bits.shape, dtype=bool)
    tkey = (b << 5) | found[0]
    tbits = int(key_inv(tkey))
    x, th = to_f32(bits, dtype), to_f32(np.array([tbits], np.uint16), dtype)[0]
    with np.errstate(invalid="ignore"):
        v = {"gt": lambda: x > th, "ge": lambda: x >= th, "key": lambda: key(bits, dtype) > tkey}[emit]()
    return tbits, v.reshape(bits.shape)


def radix_topk(bits: np.ndarray, k: int, dtype, key: Callable = class_key, rank_off: int = 0, lo_ascending: bool = False) -> np.ndarray:
    """kvz_select_topk_rows: per row the key of rank k - 1 by the same two histograms, keep key > it and, in index order, the first
    k - #(key > it) entries equal to it"""
    rows = bits.reshape(-1, bits.shape[-1])
    out = np.zeros(rows.shape, dtype=bool)
    if k <= 0 or k >= rows.shape[1]:
        out[:] = k > 0
        return out.reshape(bits.shape)
    for r in range(rows.shape[0]):
        keys = key(rows[r], dtype)
        idx = min(max(k - 1 + rank_off, 0), keys.size - 1)
        b, rank = _find_desc(np.bincount(keys >> 5, minlength=2048), idx)
        lo, _ = _find_desc(np.bincount(keys[(keys >> 5) == b] & 31, minlength=32), rank, ascending=lo_ascending)
        tkey = (b << 5) | lo
        tie = keys == tkey
        need = k - int((keys > tkey).sum())
        out[r] = (keys > tkey) | (tie & (np.cumsum(tie) <= need))
    return out.reshape(bits.shape)


# the eight faults of the audit: name -> (kwargs of radix_threshold or None, kwargs of radix_topk or None)
MUTANTS: Dict[str, Tuple[Optional[dict], Optional[dict]]] = {
    "1 sign-bit NaN ordered lowest": (dict(key=order_key_sign_only), dict(key=order_key_sign_only)),
    "2 >= in the emit": (dict(emit="ge"), None),
    "3 rank + 1": (dict(rank_off=1), None),      # (harmless in the top-k: the ties to keep are counted from the entries above the key)
    "4 rank - 1": (dict(rank_off=-1), dict(rank_off=-1)),
    "5 emit by key compare": (dict(emit="key"), None),
    "6 top-k ties by key, not by value": (None, dict(key=order_key)),
    "7 tail missing from a histogram": (dict(skip_tail="hi"), None),
    "7b tail missing from the low histogram": (dict(skip_tail="lo"), None),
    "8 low-bin search ascending": (dict(lo_ascending=True), dict(lo_ascending=True)),
}


# ---- probes ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Probe:
    name: str
    dtype: torch.dtype
    bits: np.ndarray                       # uint16 [rows, row_len]
    ratios: Tuple[float, ...]              # global-threshold ratios
    ks: Tuple[int, ...] = ()               # per-row top-k
    family: str = ""
    sweep: bool = False                    # also run across the launch geometries (bin-edge and tail probes)

    @property
    def score(self) -> torch.Tensor:
        return to_tensor(self.bits, self.dtype)


def segments(dtype) -> List[Tuple[str, int, int]]:
    """value classes from the top: (name, lowest class key, highest class key)"""
    inf = INF[dtype]
    sub = 0x03FF if dtype == F16 else 0x007F      # largest subnormal magnitude
    return [("nan", NAN_CLASS, NAN_CLASS), ("+inf", 0x8000 | inf, 0x8000 | inf), ("normal", 0x8000 | (sub + 1), 0x8000 | (inf - 1)),
            ("subnormal", 0x8001, 0x8000 | sub), ("zero", ZERO_CLASS, ZERO_CLASS), ("-subnormal", 0x7FFF - sub, 0x7FFE),
            ("-normal", 0x7FFF - (inf - 1), 0x7FFF - (sub + 1)), ("-inf", 0x7FFF - inf, 0x7FFF - inf)]


def ladder_ranks(bits: np.ndarray, dtype, n: Optional[int] = None) -> List[int]:
    """ranks that put the order statistic on the first and the last entry of every value class present (NaN block, +inf, normals,
    subnormals, zeros, negatives, -inf); ranks are capped at n - 2 (ratio < 1)"""
    ck = class_key(bits.reshape(-1), dtype)
    n = ck.size if n is None else n
    ranks, above = set(), 0
    for _, lo, hi in segments(dtype):
        c = int(((ck >= lo) & (ck <= hi)).sum())
        if c:
            ranks.update((above, above + c - 1))
        above += c
    return sorted({min(r, n - 2) for r in ranks if n >= 2})


def edge_ranks(bits: np.ndarray, dtype) -> List[int]:
    """ranks on the first and last element of the extreme populated hi bins (and those of both zeros) and, inside each, of its lowest
    and highest populated lo bins - where an off-by-one in a cumulative search shows"""
    keys = np.sort(order_key(bits.reshape(-1), dtype))[::-1]
    n = keys.size
    his = np.unique(keys >> 5)
    pick = {int(his[0]), int(his[-1]), int(his[len(his) // 2])} | ({0x8000 >> 5, 0x7FFF >> 5} & set(his.tolist()))
    finite = [h for h in his.tolist() if (h << 5) <= (0x8000 | INF[dtype])]
    if finite:
        pick.add(max(finite))
    ranks = set()
    for h in pick:
        pos = np.nonzero((keys >> 5) == h)[0]
        ranks.update((int(pos[0]), int(pos[-1])))
        los = np.unique(keys[pos] & 31)
        for lo in (int(los[0]), int(los[-1])):
            p = np.nonzero(keys == ((h << 5) | lo))[0]
            ranks.update((int(p[0]), int(p[-1])))
    return sorted({min(r, n - 2) for r in ranks if n >= 2})


def _ratios(n: int, ranks: Sequence[int]) -> Tuple[float, ...]:
    return tuple(ratio_for_rank(n, r) for r in sorted(set(ranks)))


def specials(dtype) -> np.ndarray:
    inf = INF[dtype]
    return np.array([inf + 1, 0x8000 | (inf + 1), 0x7FFF, 0xFFFF, (inf + 0x7FFF) // 2 + 1, 0x8000 | ((inf + 0x7FFF) // 2 + 1),   # NaNs
                     inf, 0x8000 | inf, 0x0000, 0x8000, 0x0001, 0x8001, inf - 1, 0x8000 | (inf - 1)], dtype=np.uint16)


def place(values: np.ndarray, rows: int, row_len: int, seed: int, placement: str, dtype) -> np.ndarray:
    """`shuffled`: a seeded permutation.  `tail`: the same, then the NaNs, infinities, zeros and extreme finite values the multiset holds
    are swapped into the last n % 8 elements (block 0's tail loop), the first element of rows and the last of rows (the scalar emit)."""
    assert values.size == rows * row_len
    out = values[np.random.default_rng(seed).permutation(values.size)].copy()
    if placement == "tail":
        n = out.size
        slots = list(range(n - (n % 8), n)) + [r * row_len for r in range(rows)] + [r * row_len + row_len - 1 for r in range(rows)]
        slots = list(dict.fromkeys(slots))
        ck = class_key(out, dtype)
        want = [int(ck.argmax()), int(ck.argmin())]                       # the largest (a NaN if any) and the smallest value
        for s in specials(dtype):
            hit = np.nonzero(out == s)[0]
            want.extend(int(h) for h in hit[:2])
        want = [w for w in dict.fromkeys(want) if w not in slots]
        for s, w in zip(slots, want):
            out[s], out[w] = out[w], out[s]
    else:
        assert placement == "shuffled", placement
    return out.reshape(rows, row_len)


def _mult(values: np.ndarray, seed: int, specials_extra: int, dtype) -> np.ndarray:
    """small multiplicities: every pattern once, one in eight twice or three times, the special patterns `specials_extra` more"""
    rng = np.random.default_rng(seed)
    pick = values[rng.random(values.size) < 0.125]
    return np.concatenate([values, pick, pick[::2], np.repeat(specials(dtype), specials_extra)])


def exhaustive_probes(dtype, seed: int = 0) -> List[Probe]:
    allp = np.arange(65536, dtype=np.uint16)
    out = []
    b = place(allp, 64, 1024, seed + 1, "shuffled", dtype)
    out.append(Probe(f"exhaustive/once/{tag(dtype)}", dtype, b, _ratios(b.size, ladder_ranks(b, dtype)) + (0.0, 1.0),
                     ks=(1, 16, 40, 500, 530, 1000, 1023), family="exhaustive"))
    m = _mult(allp, seed + 2, 3, dtype)
    rows = 11
    m = np.concatenate([m, np.repeat(specials(dtype), 2)[: (-m.size) % rows]])            # a whole number of rows
    row_len = m.size // rows
    if row_len % 8 == 0:                                                                  # keep the rows off the vector path
        m = np.concatenate([m, specials(dtype)[:rows]])
        row_len += 1
    b = place(m, rows, row_len, seed + 3, "tail", dtype)
    out.append(Probe(f"exhaustive/mult/{tag(dtype)}", dtype, b, _ratios(b.size, ladder_ranks(b, dtype) + edge_ranks(b, dtype)),
                     ks=(1, 7, row_len // 2, row_len - 1), family="exhaustive", sweep=True))
    return out


def strata_probe(dtype, rows: int = 6, seed: int = 0, placement: str = "tail") -> Probe:
    """every row holds the SAME multiset with every value class in it (placed differently per row), so one ladder of k puts the k-th
    largest of every row in the NaN block, on +inf, in the normals, the subnormals, the zeros, the negatives and on -inf"""
    inf = INF[dtype]
    rng = np.random.default_rng(seed + 100)
    sub = 0x03FF if dtype == F16 else 0x007F
    nans = np.array([inf + 1, 0x8000 | (inf + 1), 0x7FFF, 0xFFFF, inf + 2, 0x8000 | (inf + 3), 0x7E00 if dtype == F16 else 0x7FC0], np.uint16)
    normals = rng.choice(np.arange(sub + 1, inf, dtype=np.uint16), 300, replace=False)
    subs = rng.choice(np.arange(1, sub + 1, dtype=np.uint16), 40, replace=False)
    row = np.concatenate([nans, [inf] * 2, normals, normals[:30], subs, [0, 0x8000, 0, 0x8000, 0x8000], subs[:20] | 0x8000,
                          normals[:200] | 0x8000, normals[:15] | 0x8000, [0x8000 | inf] * 3]).astype(np.uint16)
    row_len = row.size + (1 if row.size % 8 == 0 else 0)
    row = np.concatenate([row, [0x3C00]])[:row_len] if row_len != row.size else row
    b = np.stack([place(row, 1, row_len, seed + 7 * r, placement if r % 2 == 0 else "shuffled", dtype)[0] for r in range(rows)])
    ks = tuple(sorted({r + 1 for r in ladder_ranks(row, dtype)} | {1, row_len - 1}))
    return Probe(f"strata/{tag(dtype)}", dtype, b, _ratios(b.size, ladder_ranks(b, dtype)), ks=ks, family="exhaustive", sweep=True)


def bin_edge_probes(dtype, seed: int = 0) -> List[Probe]:
    """multisets chosen by KEY: whole hi bins at both ends of the key space (2047: the top NaN payloads; 0: where a sign-bit NaN used to
    land; the bin of -inf, the lowest one populated today), both bins around the +-0 boundary (keys 0x7FFF / 0x8000), the bin of +inf
    and one of normals - every lo bin 0..31 of each, multiplicities 1..3; and a multiset inside ONE hi bin (the lo histogram decides)"""
    inf = INF[dtype]
    rng = np.random.default_rng(seed + 200)
    keys = np.concatenate([np.arange(h << 5, (h << 5) + 32) for h in
                           (2047, (0x8000 | inf) >> 5, 0xBC00 >> 5, 0x8000 >> 5, 0x7FFF >> 5, (0x7FFF - inf) >> 5)])
    pats = np.concatenate([key_inv(keys), np.arange(0xFFE0, 0x10000).astype(np.uint16)])       # + the patterns of the old hi bin 0
    vals = np.repeat(pats, rng.integers(1, 4, pats.size))
    vals = np.concatenate([vals, key_inv(np.array([0xBC00] * ((-vals.size) % 5 + 5)))])[: vals.size + (-vals.size) % 5]
    rows, row_len = 5, vals.size // 5
    out = []
    for placement in ("shuffled", "tail"):
        b = place(vals, rows, row_len, seed + 11, placement, dtype)
        out.append(Probe(f"bin-edge/{placement}/{tag(dtype)}", dtype, b, _ratios(b.size, edge_ranks(b, dtype) + ladder_ranks(b, dtype)),
                         ks=(1, 2, row_len // 3, row_len - 1), family="bin-edge", sweep=True))
    one = key_inv(np.arange(0xBC00, 0xBC20))                                                    # 32 normals in one hi bin
    vals = np.repeat(one, rng.integers(1, 60, 32))
    vals = np.concatenate([vals, one[:3]]) if vals.size % 8 == 0 else vals
    b = place(vals, 1, vals.size, seed + 12, "tail", dtype)
    srt = np.sort(order_key(vals, dtype))[::-1]
    firsts = [int(np.nonzero(srt == k)[0][0]) for k in np.unique(srt)]
    lasts = [int(np.nonzero(srt == k)[0][-1]) for k in np.unique(srt)]
    out.append(Probe(f"bin-edge/one-hi-bin/{tag(dtype)}", dtype, b, _ratios(b.size, [min(r, b.size - 2) for r in firsts + lasts]),
                     ks=(1, vals.size // 2, vals.size - 1), family="bin-edge", sweep=True))
    return out


def degenerate_probes(dtype, seed: int = 0) -> List[Probe]:
    inf = INF[dtype]
    rng = np.random.default_rng(seed + 300)
    one = 0x3C00 if dtype == F16 else 0x3F80
    qnan, snan = (0x7E00, 0xFE00) if dtype == F16 else (0x7FC0, 0xFFC0)
    R = (0.0, 0.1, 0.3, 0.5, 0.75, 0.9, 0.999, 1.0)
    out = []

    def add(name, vals, rows=1, ratios=R, ks=None, placement="shuffled", sweep=False):
        vals = np.asarray(vals, dtype=np.uint16)
        row_len = vals.size // rows
        b = place(vals, rows, row_len, seed + len(out), placement, dtype)
        ks = ks if ks is not None else tuple(sorted({1, max(row_len // 2, 1), max(row_len - 1, 1)}))
        out.append(Probe(f"degenerate/{name}/{tag(dtype)}", dtype, b, tuple(ratios), ks=ks, family="degenerate", sweep=sweep))

    for n in (13, 1005):                                   # all equal
        add(f"all-equal-finite/n{n}", [one] * n)
        add(f"all-zero-mixed/n{n}", [0, 0x8000] * (n // 2) + [0x8000] * (n % 2))
        add(f"all-inf/n{n}", [inf] * n)
        add(f"all-nan/n{n}", ([qnan, snan, 0x7FFF, 0xFFFF, inf + 1] * n)[:n])
    add("all-neg-inf/n21", [0x8000 | inf] * 21)
    add("one-distinct/n1005", [one] * 1004 + [inf - 1], placement="tail")
    for n in range(1, 18):                                 # n = 1..17: every split between the vector body and the tail
        vals = ([snan, inf, 0, 0x8000, qnan, 0x8000 | inf, 1, 0x8001] + list(rng.integers(0, 65536, 9)))[:n]
        add(f"tiny/n{n}", vals, ratios=(0.0, 0.2, 0.5, 0.8, 0.95), placement="tail")
    # more NaNs than the rank, exactly rank + 1 NaNs, rank + 0: m NaNs (both signs) over distinct finite values, rows of 67
    m, n = 40, 5 * 67
    fin = rng.choice(np.arange(1, inf, dtype=np.uint16), n - m, replace=False)
    vals = np.concatenate([([snan, qnan, 0xFFFF, inf + 1] * m)[:m], fin]).astype(np.uint16)
    add("nan-count/rows67", vals, rows=5, ratios=_ratios(n, [0, m - 2, m - 1, m, m + 1, n // 2, n - 2]), ks=(1, 5, 8, 9, 33, 66),
        placement="tail", sweep=True)
    return out


def poisoned_head_probes(dtype, seed: int = 0) -> List[Probe]:
    """[L, Hkv, N] scores in which one (layer, head) row of every layer is all NaN, as an inf / NaN in Q leaves a KV head
    (tests/test_gpu_score_exact.py): the product's positive canonical NaN, and the sign-bit NaN other producers write"""
    out = []
    L, Hkv, N = 3, 4, 1000
    for name, nan in (("canonical", 0x7E00 if dtype == F16 else 0x7FC0), ("sign-bit", 0xFE00 if dtype == F16 else 0xFFC0)):
        g = torch.Generator().manual_seed(seed + 400)
        s = (torch.rand(L * Hkv, N, generator=g) ** 4).to(dtype)
        b = s.view(torch.int16).numpy().view(np.uint16).copy()
        for layer in range(L):
            b[layer * Hkv + (layer + 1) % Hkv] = nan
        n, m = b.size, L * N
        out.append(Probe(f"poisoned/{name}/{tag(dtype)}", dtype, b, _ratios(n, [0, m - 1, m, m + 1, n // 2, n - 2]) + (0.1, 0.3, 0.6),
                         ks=(1, 300, 999), family="poisoned"))
    return out


def all_probes(dtype, seed: int = 0) -> List[Probe]:
    return (exhaustive_probes(dtype, seed) + [strata_probe(dtype, seed=seed)] + bin_edge_probes(dtype, seed) + degenerate_probes(dtype, seed)
            + poisoned_head_probes(dtype, seed))


def fixture_probes(dtype) -> List[Probe]:
    """what tests/golden/g16_select_specials.npz records from the reference: the exhaustive and the degenerate probes (without the
    exhaustive probe with multiplicities: its masks alone would take the fixture past the size a committed file may have)"""
    return [p for p in all_probes(dtype) if p.family in ("exhaustive", "degenerate") and "/mult/" not in p.name]


def fixture_key(p: Probe, what: str, x) -> str:
    return f"{p.name}/{what}/{x!r}"
