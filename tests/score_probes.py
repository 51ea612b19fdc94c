"""Scoring probes whose correct 16-bit scores are known EXACTLY (host-only helpers of the exact scoring tests).

The random-input scoring tests compare with the oracle under fixed bounds (``conftest.check_score_parity``: up to 0.2 % of fp16
scores not bit-identical, any score up to 8 grid steps off).  One key counted twice or dropped in one row's l_r moves only the scores
whose column maximum comes from that row, by a step or two: inside those bounds.  These inputs make every logit either 0 ("live") or
at most -181 ("dead", exp of it is exactly 0 in fp32), so every live p is exp(0) = 1, l_r is an exact integer count whatever the
accumulation order, and the score of ctx key j is

    score_j = half(1 / min{ l_r : key j is live for row r })        (0 when j is live for no row)

Construction (per KV head; row r = (g, i) is query head h*G + g at position i, r = g * q_len + i):
  * every query row is two-hot: 1.0 in dims a and b.  The pair {a, b} is the row's class.  Background rows share the class {0, 1};
    a witnessed row has a class of its own, drawn from dims 2 .. D-1;
  * every K entry is 0 or DEAD (-2048).  A key is live for class {a, b} iff k[a] == k[b] == 0: the dot product is then 0, -2048 or
    -4096, exact in fp32 / fp16 / bf16, and after the rounding chain 0 or <= -181;
  * a witness key of row r is DEAD in every dim but r's pair: live for r alone.  Dropping it from l_r, counting it twice, or losing
    the pair (r, j) in the column maximum moves score_j;
  * repeat key p is live for the witnessed rows at position p (their diagonal, counted) and p - 1 (beyond their causal limit, not
    counted), and key 0 for the background class;
  * keys the scoring call must not read (between the sink and the chunk, between the chunk and the repeat chunk, slack rows behind the
    K head) are all 0: live for every row, so reading one moves l_r of every row;
  * hot variant: the sink keys are all 0 (live for every row: each row's first key block holds its maximum).  Cold variant: the sink
    is live for the background class only, so a witnessed row's first key block is dead, its pass-A reference sits at -181 or below,
    and its live key lies 181 or more above it (the redo loop of the key-per-lane pass).  Cold also has rows with l = 1 (score 1.0).

Safe counts.  The kernels do not compute 1 / l: pass A sums exp2(0) = 1 exactly and the merge returns log l_r = logf(Lp) (delta = 0
when m_r = 0), pass B takes t = (0 - 0) - log l_r, the finalize returns half(expf(t)).  For l < 2^11, |ln l| < 8, so one fp32 ulp of
log l is at most 2^-21 absolute; logf, the subtraction and expf together stay well inside a relative error of 2^-18.  A count is SAFE
when half(1 / l) is the same for every value within a relative 2^-16 of 1 / l (four times that budget); every count a score depends on
is checked.  A witnessed row's count must also be DISTINGUISHABLE: half(1/(l-1)), half(1/l) and half(1/(l+1)) all differ.  Both hold
for every l <= 64 in both dtypes; the helpers check each count exactly with rational arithmetic.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import torch

DEAD = -2048.0
BG = (0, 1)                 # class of the background rows
SAFE_REL = Fraction(1, 1 << 16)
PA_ROWS = 256               # rows per unit of the pass-A partition (kvz_score.hip)
SC_TILE = 128               # keys per pass-A key tile
MAX_WITNESS_L = 64
MAX_KEYS_PER_ROW = 16        # ctx keys live for one witnessed row


# ---- exact 16-bit rounding of a positive rational ------------------------------------------------------------------------------
def _mant(dtype) -> int:
    return 10 if dtype == torch.float16 else 7


def round16(v: Fraction, dtype) -> Fraction:
    """v > 0 (normal range of both formats) rounded to nearest even on the grid of `dtype`."""
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    if Fraction(2) ** (e + 1) <= v:
        e += 1
    ulp = Fraction(2) ** (e - _mant(dtype))
    q = v / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return n * ulp


@lru_cache(maxsize=None)
def count_is_safe(l: int, dtype) -> bool:
    """half(1/l) is the same for every value within a relative SAFE_REL of 1/l (rounding is monotone: the two ends decide)."""
    v = Fraction(1, l)
    r = round16(v, dtype)
    return round16(v * (1 - SAFE_REL), dtype) == r == round16(v * (1 + SAFE_REL), dtype)


@lru_cache(maxsize=None)
def count_is_distinguishable(l: int, dtype) -> bool:
    """half(1/(l-1)), half(1/l), half(1/(l+1)) all differ (l = 1: half(1) and half(1/2) differ)."""
    vals = {round16(Fraction(1, n), dtype) for n in (l - 1, l, l + 1) if n >= 1}
    return len(vals) == (3 if l > 1 else 2)


def inv16(l: torch.Tensor, dtype) -> torch.Tensor:
    """half(1/l) for integer counts l >= 1 (0 -> 0).  Through fp32: exact for every SAFE count (fp32 rounding moves 1/l by at most
    2^-24 relative, and a safe count has no 16-bit rounding boundary within 2^-16 of 1/l)."""
    lf = l.to(torch.float64)
    v = torch.where(lf > 0, 1.0 / lf.clamp_min(1), torch.zeros_like(lf))
    return v.to(torch.float32).to(dtype)


# ---- the pass-A partition (host code of the library, no GPU needed) -------------------------------------------------------------
def score_plan(sink: int, m: int, q_len: int, G: int, Hkv: int) -> Tuple[List[Tuple[int, int]], int]:
    """kvz_debug_score_plan: [(unit, key tile)] where each of the nb blocks of the row-statistics pass starts, and nb."""
    import ctypes as C
    from kvzip_amd import _lib
    lib = _lib.load()
    unit, tile = (C.c_uint16 * 257)(), (C.c_uint16 * 257)()
    nb, max_seg, rows = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib.kvz_debug_score_plan(sink, m, q_len, G, Hkv, unit, tile, C.byref(nb), C.byref(max_seg), C.byref(rows))
    assert rc == 0 and rows.value == PA_ROWS, (rc, rows.value)
    return [(int(unit[b]), int(tile[b])) for b in range(nb.value)], nb.value


# ---- the probe -------------------------------------------------------------------------------------------------------------------
@dataclass
class ScoreProbe:
    q: torch.Tensor              # [1, H, q_len, D]
    k_store: torch.Tensor        # [1, Hkv, klen + slack, D]; the scoring call sees k = k_store[:, :, :klen]
    klen: int
    sink: int
    start: int
    end: int
    variant: str
    cls: torch.Tensor            # [Hkv, R, 2] class (dims a, b) of every row
    l: torch.Tensor              # [Hkv, R] int64 exact row counts l_r
    minl: torch.Tensor           # [Hkv, m] int64 min l_r over the rows a ctx key is live for (0: live for none)
    want: torch.Tensor           # [Hkv, m] expected scores (dtype)
    witness_rows: Dict[str, List[Tuple[int, int]]] = field(default_factory=dict)   # kind -> [(h, r)]
    witness_keys: Dict[str, List[Tuple[int, int]]] = field(default_factory=dict)   # kind -> [(h, j)]

    @property
    def k(self) -> torch.Tensor:
        return self.k_store[:, :, :self.klen]

    @property
    def dtype(self):
        return self.q.dtype

    @property
    def m(self) -> int:
        return self.end - self.start

    @property
    def q_len(self) -> int:
        return self.q.shape[2]

    @property
    def shape(self):
        _, H, q_len, D = self.q.shape
        Hkv = self.k_store.shape[1]
        return H, Hkv, H // Hkv, q_len, D

    def all_witness_rows(self) -> List[Tuple[int, int]]:
        return sorted({x for v in self.witness_rows.values() for x in v})

    def all_witness_keys(self) -> List[Tuple[int, int]]:
        return sorted({x for v in self.witness_keys.values() for x in v})


def _key_edges(sink: int, m: int, plan_keys: Sequence[int]) -> Dict[str, List[int]]:
    """ctx keys where the kernels cut: first / last key, 32-key blocks of the virtual key stream (pass A) and of the chunk (pass B,
    group bounds), the sink / chunk seam, and the key-tile cuts of the pass-A partition."""
    out = {"first_last": sorted({0, m - 1}),
           "block32_virtual": [j for j in range(m) if (sink + j) % 32 in (0, 31)],
           "block32_ctx": [j for j in range(m) if j % 32 in (0, 31)],
           "seam": [j for j in (32 - sink % 32 - 1, 32 - sink % 32) if sink % 32 and 0 <= j < m],
           "plan_cut": sorted({j for j in plan_keys if 0 <= j < m})}
    return out


def _row_edges(G: int, q_len: int, plan_rows: Sequence[int]) -> Dict[str, List[int]]:
    R = G * q_len
    last = R - 1
    return {"query_head_ends": sorted({g * q_len + i for g in range(G) for i in (0, q_len - 1)}),
            "unit256": sorted({r for r in range(R) if r % PA_ROWS in (0, PA_ROWS - 1)} | {last}),
            "plan_cut": sorted(set(plan_rows)),
            # rows whose causal limit (virtual key sink + m + i) sits on a 32-key block edge, in the first and the last query head
            "causal_edge": [],
            "group32": sorted({r for r in range(R) if r % 32 in (0, 31)} | {last})}


def score_probe(Hkv: int, G: int, q_len: int, D: int, dtype, sink: int, start: int, m: int, variant: str = "hot",
                tail_gap: int = 0, slack: int = 0, seed: int = 0, plan: Optional[List[Tuple[int, int]]] = None,
                max_witness_rows: Optional[int] = None) -> ScoreProbe:
    """Builds the probe of one scoring call (see the module docstring).  `plan`: the pass-A block starts (score_plan; None = ask the
    library); `tail_gap`: keys between the chunk and the repeat chunk; `slack`: rows behind each K head (all 0) that must not be read."""
    assert variant in ("hot", "cold") and D in (64, 128) and start >= sink and m >= 1
    end = start + m
    klen = end + tail_gap + q_len
    R = G * q_len
    gen = torch.Generator().manual_seed(seed * 7919 + Hkv * 131 + G * 17 + q_len + m)
    if plan is None:
        plan, _ = score_plan(sink, m, q_len, G, Hkv)
    n_bulk = 0 if m < 8 else 4
    pairs_all = [(a, b) for a in range(2, D) for b in range(a + 1, D)]

    K = torch.zeros(Hkv, klen + slack, D)            # unseen keys and slack rows: 0 (live for every row)
    Q = torch.zeros(Hkv, R, D)
    cls = torch.zeros(Hkv, R, 2, dtype=torch.long)
    witness_rows: Dict[str, List[Tuple[int, int]]] = {}
    witness_keys: Dict[str, List[Tuple[int, int]]] = {}
    rep0 = klen - q_len
    for h in range(Hkv):
        # pass-A cuts inside a unit of this head: rows of that row tile, ctx keys at the cut
        plan_rows, plan_keys = [], []
        for u, t in plan:
            if t > 0 and u % Hkv == h:
                rt = u // Hkv
                plan_rows += [rt * PA_ROWS, min(R - 1, rt * PA_ROWS + PA_ROWS - 1)]
                v = t * SC_TILE - sink
                plan_keys += [v - 1, v]
        kedge = _key_edges(sink, m, plan_keys)
        redge = _row_edges(G, q_len, plan_rows)
        lim = [i for i in range(q_len) if (sink + m + i) % 32 in (0, 31)]
        redge["causal_edge"] = sorted({g * q_len + i for g in {0, G - 1} for i in lim})
        # bulk keys: live for the background class; spread over the chunk, away from the witnessed keys
        wk_set = {j for v in kedge.values() for j in v}
        spare = [j for j in range(m) if j not in wk_set]
        perm = torch.randperm(len(spare), generator=gen).tolist()
        spare = [spare[i] for i in perm]
        bulk, spare = spare[:n_bulk], spare[n_bulk:]
        # witnessed rows in priority order, as many as there are ctx keys to witness them (and classes)
        order = ["query_head_ends", "plan_cut", "unit256", "causal_edge", "group32"]
        rows: List[int] = []
        kind_of: Dict[int, List[str]] = {}
        for kind in order:
            for r in redge[kind]:
                kind_of.setdefault(r, []).append(kind)
                if r not in rows:
                    rows.append(r)
        keys_pool = [j for kind in ("first_last", "seam", "plan_cut", "block32_virtual", "block32_ctx") for j in kedge[kind]]
        keys_pool = list(dict.fromkeys(keys_pool)) + spare
        cap = min(len(keys_pool), len(pairs_all))
        if max_witness_rows is not None:
            cap = min(cap, max_witness_rows)
        rows = rows[:cap]
        # classes: background {0, 1}; a shuffled pair per witnessed row (different per head)
        cls[h, :, 0], cls[h, :, 1] = BG[0], BG[1]
        pp = torch.randperm(len(pairs_all), generator=gen)[:len(rows)].tolist()
        for n, r in enumerate(rows):
            cls[h, r, 0], cls[h, r, 1] = pairs_all[pp[n]][0], pairs_all[pp[n]][1]
        # ctx keys: one per witnessed row (the witnessed edge keys first), the witnessed edge keys left over go round-robin
        Kh = K[h]
        Kh[start:end] = DEAD
        wkeys = keys_pool[:len(rows)]
        extra = [j for j in keys_pool[len(rows):] if j in wk_set]
        owner: Dict[int, int] = {}
        for n, j in enumerate(wkeys):
            owner[j] = rows[n]
        per_row = {r: 1 for r in rows}
        for n, j in enumerate(extra):   # (a row keeps at most MAX_KEYS_PER_ROW: the rest stay dead)
            r = rows[n % len(rows)] if rows else None
            if r is not None and per_row[r] < MAX_KEYS_PER_ROW:
                owner[j] = r
                per_row[r] += 1
        for j, r in owner.items():
            if r is None:
                continue
            a, b = int(cls[h, r, 0]), int(cls[h, r, 1])
            Kh[start + j, a] = 0.0
            Kh[start + j, b] = 0.0
        for j in bulk:
            Kh[start + j, BG[0]] = 0.0
            Kh[start + j, BG[1]] = 0.0
        # sink: hot = live for every row; cold = live for the background class only
        if sink:
            if variant == "cold":
                Kh[:sink] = DEAD
                Kh[:sink, BG[0]] = 0.0
                Kh[:sink, BG[1]] = 0.0
        # repeat chunk: key 0 live for the background; diagonal (counted) and diagonal + 1 (beyond the causal limit) per witnessed row.
        # Cold: every other witnessed row has no live diagonal (l = 1 for a row with one ctx key)
        Kh[rep0:klen] = DEAD
        Kh[rep0, BG[0]] = 0.0
        Kh[rep0, BG[1]] = 0.0
        for n, r in enumerate(rows):
            i = r % q_len
            a, b = int(cls[h, r, 0]), int(cls[h, r, 1])
            if not (variant == "cold" and n % 2 == 1):
                Kh[rep0 + i, a] = 0.0
                Kh[rep0 + i, b] = 0.0
            if i + 1 < q_len:
                Kh[rep0 + i + 1, a] = 0.0
                Kh[rep0 + i + 1, b] = 0.0
        Q[h, torch.arange(R), cls[h, :, 0]] = 1.0
        Q[h, torch.arange(R), cls[h, :, 1]] = 1.0
        # witness records
        rows_set = set(rows)
        for r in rows:
            for kind in kind_of[r]:
                witness_rows.setdefault(kind, []).append((h, r))
        for kind, js in kedge.items():
            for j in js:
                if owner.get(j) is not None:
                    witness_keys.setdefault(kind, []).append((h, j))
        witness_keys.setdefault("dead_for_all", []).extend(
            (h, j) for j in range(m) if j not in owner and j not in bulk)
        witness_keys.setdefault("bulk_ties", []).extend((h, j) for j in bulk)
        assert rows_set == {owner[j] for j in wkeys}

    q = Q.view(Hkv, G, q_len, D).reshape(1, Hkv * G, q_len, D).to(dtype)
    k_store = K.unsqueeze(0).to(dtype)
    l, minl = exact_counts(q, k_store[:, :, :klen], sink, start, end)
    p = ScoreProbe(q, k_store, klen, sink, start, end, variant, cls, l, minl, inv16(minl, dtype), witness_rows, witness_keys)
    _check(p)
    return p


def live_by_class(q: torch.Tensor, k: torch.Tensor, sink: int, start: int, end: int, h: int):
    """(classes [C, 2], row -> class index [R], live [C, n_keys] over the keys the call sees: sink ++ chunk ++ repeat chunk)."""
    _, H, q_len, D = q.shape
    Hkv, klen = k.shape[1], k.shape[2]
    G = H // Hkv
    Qh = q[0, h * G:(h + 1) * G].reshape(G * q_len, D).float()
    two = Qh.nonzero()
    assert two.shape[0] == 2 * G * q_len and bool((Qh.sum(-1) == 2).all()), "every query row must be two-hot"
    pair = two[:, 1].view(-1, 2)
    classes, inv = torch.unique(pair, dim=0, return_inverse=True)
    kh = k[0, h].float()
    keys = torch.cat([kh[:sink], kh[start:end], kh[klen - q_len:]], dim=0)
    assert bool(((keys == 0) | (keys == DEAD)).all())
    z = keys == 0
    live = z[:, classes[:, 0]] & z[:, classes[:, 1]]          # [n_keys, C]
    return classes, inv, live.t().contiguous()


def exact_counts(q: torch.Tensor, k: torch.Tensor, sink: int, start: int, end: int, causal_shift: int = 0,
                 drop: Optional[Tuple[int, int, int]] = None, l_delta: Optional[Tuple[int, int, int]] = None):
    """Exact l_r [Hkv, R] and, per ctx key, the minimum l_r over the rows it is live for [Hkv, m] (0: none), computed from the inputs
    themselves.  Fault injection for the audit: `causal_shift` moves every row's causal limit; `drop` = (h, r, j) removes the pair
    (row r, ctx key j) from both passes; `l_delta` = (h, r, d) adds d to l_r."""
    _, H, q_len, D = q.shape
    Hkv = k.shape[1]
    G = H // Hkv
    R, m = G * q_len, end - start
    L = torch.zeros(Hkv, R, dtype=torch.long)
    MIN = torch.zeros(Hkv, m, dtype=torch.long)
    big = 1 << 40
    i_of = torch.arange(R) % q_len
    for h in range(Hkv):
        classes, inv, live = live_by_class(q, k, sink, start, end, h)
        base = live[:, :sink + m].sum(-1)                                        # [C]
        rep = live[:, sink + m:].long().cumsum(-1)                               # [C, q_len]: repeat keys 0..p live
        lim = (i_of + causal_shift).clamp(-1, q_len - 1)
        l = base[inv] + torch.where(lim >= 0, rep[inv, lim.clamp_min(0)], torch.zeros_like(lim))
        ctx = live[:, sink:sink + m]                                             # [C, m]
        if drop is not None and drop[0] == h and bool(ctx[inv[drop[1]], drop[2]]):
            l[drop[1]] -= 1
        if l_delta is not None and l_delta[0] == h:
            l[l_delta[1]] += l_delta[2]
        L[h] = l
        # min over the rows of each class, then over the classes a key is live for
        cmin = torch.full((classes.shape[0],), big, dtype=torch.long).scatter_reduce(0, inv, l, "amin")
        mn = torch.where(ctx, cmin[:, None], torch.full((), big)).amin(0)
        if drop is not None and drop[0] == h:
            _, r, j = drop
            rows_j = ctx[inv, j].clone()                                         # [R]: the rows key j is live for, without r
            rows_j[r] = False
            mn[j] = l[rows_j].min() if bool(rows_j.any()) else big
        MIN[h] = torch.where(mn >= big, torch.zeros_like(mn), mn)
    return L, MIN


def expected_under(p: ScoreProbe, **fault) -> torch.Tensor:
    _, minl = exact_counts(p.q, p.k, p.sink, p.start, p.end, **fault)
    return inv16(minl.clamp_min(0), p.dtype)


def _check(p: ScoreProbe):
    """Every count a score depends on is safe, every row has a live key (its maximum is 0), every witnessed row's count is small and
    distinguishable, and every witnessed key is live for exactly one row."""
    assert int(p.l.min()) >= 1, "a row without a live key"
    for l in sorted(set(p.minl[p.minl > 0].tolist())):
        assert count_is_safe(l, p.dtype), ("unsafe count", l)
    for h, r in p.all_witness_rows():
        l = int(p.l[h, r])
        assert l <= MAX_WITNESS_L and count_is_distinguishable(l, p.dtype), ("witnessed row count", h, r, l)


def bits_equal(got: torch.Tensor, want: torch.Tensor) -> Tuple[bool, int]:
    """(equal, number of differing 16-bit patterns); NaN never equals."""
    g = got.detach().cpu().contiguous().view(torch.int16)
    w = want.detach().cpu().contiguous().view(torch.int16)
    assert g.shape == w.shape, (g.shape, w.shape)
    n = int((g != w).sum())
    return n == 0, n


def describe_mismatch(p: ScoreProbe, got: torch.Tensor, limit: int = 8) -> str:
    """The first differing scores with the count the probe expects and the count the kernel's value implies (1 / score)."""
    g = got.detach().cpu().float().reshape(p.want.shape)
    w = p.want.float()
    bad = ((g != w) | g.isnan()).nonzero().tolist()
    lines = [f"{len(bad)} of {w.numel()} scores differ"]
    for h, j in bad[:limit]:
        gv = float(g[h, j])
        lines.append(f"  head {h} ctx key {j}: got {gv!r} (1/got = {1 / gv if gv else float('inf'):.3f}), want {float(w[h, j])!r} "
                     f"(min l = {int(p.minl[h, j])})")
    return "\n".join(lines)
