"""CPU self-check of the exact scoring probes (tests/score_probes.py) that tests/test_gpu_score_exact.py compares the kernels with bit for bit:
1. the CPU oracle (both its forms: the reference's half softmax and the explicit fp32 chain) returns the predicted scores bit for bit;
2. every count a score depends on is safe, and the rational rounding behind that check agrees with the conversions of numpy / torch;
3. a fault audit: one key dropped from or added to a witnessed row's l_r, a witnessed (row, key) pair lost, or the causal limit moved by
   one changes an expected score - the faults the fixed parity bounds of the random-input tests let through."""
import numpy as np
import pytest
import torch

import kvzip_oracle as orc
import score_probes as sp

F16, BF16 = torch.float16, torch.bfloat16

# (Hkv, G, q_len, D, sink, start, m, tail_gap, slack)
SMALL = [
    (2, 3, 40, 64, 4, 10, 100, 3, 5),        # sink not a multiple of 32, keys between sink / chunk / repeat chunk, slack rows
    (2, 3, 40, 64, 0, 0, 100, 0, 0),         # no sink
    (1, 7, 33, 128, 30, 40, 70, 5, 8),       # G = 7: 32-row groups across query heads
    (2, 2, 300, 128, 32, 32, 300, 0, 0),     # several pass-A units and blocks, causal limits on many key blocks
    (1, 1, 1, 64, 0, 0, 1, 0, 0),            # one row, one key
    (3, 1, 7, 128, 4, 4, 3, 2, 3),           # G = 1, m = 3
]


def _name(geom, dtype, variant):
    return f"{variant}/{str(dtype)[6:]}/Hkv{geom[0]}G{geom[1]}q{geom[2]}D{geom[3]}s{geom[4]}m{geom[6]}"


def _probe(geom, dtype, variant):
    Hkv, G, q_len, D, sink, start, m, gap, slack = geom
    return sp.score_probe(Hkv, G, q_len, D, dtype, sink, start, m, variant, tail_gap=gap, slack=slack, seed=q_len)


@pytest.mark.parametrize("variant", ["hot", "cold"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("geom", SMALL, ids=[f"g{i}" for i in range(len(SMALL))])
def test_probe_scores_equal_the_oracle_bit_for_bit(geom, dtype, variant):
    p = _probe(geom, dtype, variant)
    a = orc.get_score(p.q, p.k.contiguous(), p.sink, p.start, p.end)[0]
    b = orc.get_score_chain_fp32(p.q, p.k.contiguous(), p.sink, p.start, p.end)[0]
    assert sp.bits_equal(a, p.want)[0], sp.describe_mismatch(p, a)
    assert sp.bits_equal(b, p.want)[0], sp.describe_mismatch(p, b)
    # what the probe is made of: every row has a live key, witnessed keys score half(1/l) of their row, dead keys 0
    assert int(p.l.min()) >= 1
    for h, j in p.witness_keys.get("dead_for_all", []):
        assert float(p.want[h, j]) == 0.0
    if variant == "cold" and geom[2] > 1:
        assert bool((p.want == 1.0).any()), "cold probes hold rows with l = 1"


def test_probe_requirements_at_the_headline_shape():
    """the headline first chunk: every witness class present, witnessed rows small and distinguishable, unique classes"""
    p = sp.score_probe(4, 7, 2013, 128, F16, 32, 32, 2000, "cold")
    for kind in ("query_head_ends", "unit256", "plan_cut", "causal_edge", "group32"):
        assert p.witness_rows.get(kind), kind
    for kind in ("first_last", "block32_virtual", "block32_ctx", "plan_cut", "dead_for_all", "bulk_ties"):
        assert p.witness_keys.get(kind), kind
    rows = p.all_witness_rows()
    assert len(rows) >= 4 * 800
    for h in range(4):
        wr = [r for hh, r in rows if hh == h]
        assert len({tuple(p.cls[h, r].tolist()) for r in wr}) == len(wr), "witnessed rows need classes of their own"
    # background rows share one count: groups with equal n_r (the ties of the group bounds)
    bg = (p.cls[..., 0] == sp.BG[0]) & (p.cls[..., 1] == sp.BG[1])
    assert len(set(p.l[bg].tolist())) == 1


def test_safe_counts():
    # small counts are safe and distinguishable in both dtypes; the checks flag what they should
    for dtype in (F16, BF16):
        for l in range(1, sp.MAX_WITNESS_L + 1):
            assert sp.count_is_safe(l, dtype) and sp.count_is_distinguishable(l, dtype), (dtype, l)
    assert not sp.count_is_safe(65, F16)           # 1/65 lies within 2^-16 of an fp16 rounding boundary
    assert not sp.count_is_safe(255, BF16)
    assert not sp.count_is_distinguishable(1464, F16) and not sp.count_is_distinguishable(190, BF16)
    # the rational rounding agrees with numpy's correctly rounded fp64 -> fp16 and with inv16 for every safe count
    ls = torch.arange(1, 2049)
    got16 = sp.inv16(ls, F16)
    gotb = sp.inv16(ls, BF16)
    for l in range(1, 2049):
        r16 = sp.round16(sp.Fraction(1, l), F16)
        assert float(np.float16(1.0 / l)) == float(r16)
        if sp.count_is_safe(l, F16):
            assert float(got16[l - 1]) == float(r16), l
        if sp.count_is_safe(l, BF16):
            assert float(gotb[l - 1]) == float(sp.round16(sp.Fraction(1, l), BF16)), l
    # the probes refuse a witnessed row whose count is not distinguishable
    p = sp.score_probe(1, 1, 1, 64, BF16, 0, 0, 1, "hot")
    p.l[0, 0] = 190
    with pytest.raises(AssertionError):
        sp._check(p)


def _audit(p):
    """{fault class: (cases, cases that change an expected score)}"""
    base = p.want
    res = {}

    def rec(kind, moved):
        n, k = res.get(kind, (0, 0))
        res[kind] = (n + 1, k + int(moved))

    for h, r in p.all_witness_rows():
        for d in (-1, 1):
            w = sp.expected_under(p, l_delta=(h, r, d))
            rec(f"row l{d:+d}", not torch.equal(w.view(torch.int16), base.view(torch.int16)))
    for kind, keys in p.witness_keys.items():
        if kind in ("dead_for_all", "bulk_ties"):   # (live for no row / for many rows with one count: the ties, not a witness)
            continue
        for h, j in keys:
            # the row that holds the column maximum of key j (the smallest count among the rows it is live for)
            classes, inv, live = sp.live_by_class(p.q, p.k, p.sink, p.start, p.end, h)
            rows = live[inv, p.sink + j].nonzero().flatten()
            r = int(rows[p.l[h, rows].argmin()])
            w = sp.expected_under(p, drop=(h, r, j))
            rec(f"key drop/{kind}", int(w[h, j].view(torch.int16)) != int(base[h, j].view(torch.int16)))
    for s in (-1, 1):
        w = sp.expected_under(p, causal_shift=s)
        rec(f"causal {s:+d}", not torch.equal(w.view(torch.int16), base.view(torch.int16)))
    return res


@pytest.mark.parametrize("variant", ["hot", "cold"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_fault_audit(dtype, variant):
    rows = []
    for geom in SMALL[:4] + SMALL[5:]:
        p = _probe(geom, dtype, variant)
        for kind, (n, moved) in _audit(p).items():
            rows.append((_name(geom, dtype, variant), kind, n, moved))
    print("\nFAULT AUDIT (expected scores recomputed exactly with the fault injected)")
    print(f"{'probe':<40}{'fault':<28}{'cases':>7}{'moved':>7}")
    for name, kind, n, moved in rows:
        print(f"{name:<40}{kind:<28}{n:>7}{moved:>7}")
    assert all(n == moved for _, _, n, moved in rows), [r for r in rows if r[2] != r[3]]
    kinds = {r[1] for r in rows}
    assert {"row l-1", "row l+1", "causal -1", "causal +1", "key drop/first_last", "key drop/block32_ctx",
            "key drop/block32_virtual", "key drop/plan_cut"} <= kinds, kinds
    assert "key drop/seam" in kinds
