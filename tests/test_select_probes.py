"""CPU self-check of the selection probes (tests/select_probes.py) that tests/test_gpu_select_values.py runs the kernels on:
1. what a probe expects BY COUNTING equals the reference's expressions evaluated by torch on the CPU (sort descending, score > thres,
   torch.topk; attention/score.py:93-97, 112-114), with NaN == NaN and +0 == -0 as value classes, and equals every oracle:
   orc.threshold, orc.threshold_heads, orc.threshold_uniform, the C oracle;
2. the oracle and the counting are pinned to what the REFERENCE itself returned (tests/golden/g16_select_specials.npz);
3. the numpy restatement of the kernels' radix selection agrees with the counting, and a fault audit: each of eight faults injected
   into the restatement changes what at least one probe expects, for each dtype."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import kvzip_oracle as orc
import select_probes as sp
from conftest import ROOT, check_uniform_contract, load_golden

DT = pytest.mark.parametrize("dtype", sp.DTYPES, ids=["f16", "bf16"])
_cache = {}


def probes(dtype):
    if dtype not in _cache:
        _cache[dtype] = sp.all_probes(dtype)
    return _cache[dtype]


def _thres_bits(x: float, dtype) -> int:
    return sp.f32_to_bits(x, dtype)


@DT
def test_probe_families_hold_what_they_declare(dtype):
    ps = probes(dtype)
    names = [p.name for p in ps]
    assert len(set(names)) == len(names)
    ex = next(p for p in ps if p.name.startswith("exhaustive/once"))
    assert np.array_equal(np.sort(ex.bits.reshape(-1)), np.arange(65536, dtype=np.uint16))
    mult = next(p for p in ps if p.name.startswith("exhaustive/mult"))
    cnt = np.bincount(mult.bits.reshape(-1), minlength=65536)
    assert cnt.min() >= 1 and cnt.max() >= 3 and mult.bits.size % 8 != 0 and mult.bits.shape[1] % 8 != 0
    # the ladder of the exhaustive probes puts the rank in every value class, both zeros' boundary included
    for p in (ex, mult):
        seen = set()
        ck = sp.class_key(p.bits, dtype)
        for r in p.ratios:
            if r < 1:
                t, _ = sp.class_at_rank(ck, sp.rank_of_ratio(p.bits.size, r))
                seen.update(name for name, lo, hi in sp.segments(dtype) if lo <= t <= hi)
        want = {s[0] for s in sp.segments(dtype)} - ({"-inf"} if p is ex else set())   # (the single -inf is rank n - 1: ratio 1)
        assert want <= seen, (p.name, want - seen)
    # tail placement: the last n % 8 elements and the row starts hold specials
    assert sp.is_nan(mult.bits.reshape(-1)[-(mult.bits.size % 8):], dtype).any()
    one = next(p for p in ps if "one-hi-bin" in p.name)
    assert len(np.unique(sp.order_key(one.bits, dtype) >> 5)) == 1
    tiny = [p for p in ps if "/tiny/" in p.name]
    assert sorted(p.bits.size for p in tiny) == list(range(1, 18))
    for p in ps:
        if p.family == "poisoned":
            assert (sp.is_nan(p.bits, dtype).all(-1).reshape(3, 4).sum(-1) == 1).all()


@DT
def test_counting_equals_the_reference_expressions_and_the_oracles(dtype):
    """global threshold: counting == sort / > of the reference == orc.threshold (mask bit for bit, kept, threshold as a number)"""
    for p in probes(dtype):
        score = p.score
        for r in p.ratios:
            e = sp.expect_threshold(p.bits, r, dtype)
            rv, rt = sp.ref_threshold(score, r)
            ov, ot = orc.threshold(score, r)
            assert np.array_equal(rv.numpy(), e.valid), (p.name, r, "reference")
            assert np.array_equal(ov.numpy(), e.valid), (p.name, r, "oracle")
            assert sp.same_class(_thres_bits(rt, dtype), e.thres_bits, dtype), (p.name, r, rt, hex(e.thres_bits))
            assert sp.same_class(_thres_bits(ot, dtype), e.thres_bits, dtype), (p.name, r, ot, hex(e.thres_bits))
            assert e.kept == int(rv.sum()) and np.array_equal(e.row_counts, rv.sum(-1).int().numpy().reshape(-1))
            # and the restatement of the kernels, with the kernels' key
            tb, v = sp.radix_threshold(p.bits, r, dtype)
            assert np.array_equal(v, e.valid) and sp.same_class(tb, e.thres_bits, dtype), (p.name, r, "restatement")
            # ... whose per-row top-k key treats the classes alike
            tb, v = sp.radix_threshold(p.bits, r, dtype, key=sp.class_key)
            assert np.array_equal(v, e.valid) and sp.same_class(tb, e.thres_bits, dtype), (p.name, r, "restatement, class key")


@DT
def test_counting_equals_the_reference_topk_and_the_uniform_oracle(dtype):
    """per-row top-k: exactly k per row, the reference's kept multiset by value class, lowest index among equals; orc.threshold_uniform
    bit for bit.  conftest.check_uniform_contract serves wherever no kept value is a NaN (torch.equal of NaNs is false there)."""
    for p in probes(dtype):
        score = p.score
        N = p.bits.shape[-1]
        for k in p.ks:
            if not 0 < k < N:
                continue
            e = sp.expect_topk(p.bits, k, dtype)
            rv = sp.ref_topk(score, k).numpy()
            moved = sp.check_topk_contract(f"{p.name}/k{k}", p.bits, e, rv, k, dtype)
            if not sp.is_nan(p.bits, dtype).any():
                assert moved == check_uniform_contract(f"{p.name}/k{k}", score, torch.from_numpy(e), torch.from_numpy(rv), k)
            # lowest index among the entries equal AS NUMBERS to the boundary value
            ck = sp.class_key(p.bits, dtype)
            for i in range(p.bits.shape[0]):
                t, _ = sp.class_at_rank(ck[i], k - 1)
                tie = np.nonzero(ck[i] == t)[0]
                kept = e[i][tie]
                assert not (np.diff(kept.astype(int)) > 0).any(), (p.name, k, i)
            assert np.array_equal(sp.radix_topk(p.bits, k, dtype), e), (p.name, k, "restatement")
            # the oracle, at a ratio that gives this k
            ratio = (k + 0.5) / N
            assert int(N * ratio) == k
            ov, _ = orc.threshold_uniform([score], ratio)
            assert np.array_equal(ov[0].numpy(), e), (p.name, k, "orc.threshold_uniform")


@DT
@pytest.mark.parametrize("n_ctx", [1, 7, 131072])
def test_counting_equals_the_head_level_oracle(dtype, n_ctx):
    for p in probes(dtype):
        if p.bits.size > 4096:
            continue
        for r in p.ratios + (0.05, 0.5):
            e = sp.expect_heads(p.bits, n_ctx, r, dtype)
            ov, ot = orc.threshold_heads(p.score, n_ctx, r)
            assert np.array_equal(ov.numpy(), e.valid), (p.name, r)
            assert sp.same_class(_thres_bits(ot, dtype), e.thres_bits, dtype), (p.name, r)
            if n_ctx == 7:                                  # the expansion itself (model/wrapper.py:54-57), through the reference's lines
                rv, rt = sp.ref_threshold(p.score.unsqueeze(-1).expand(*p.bits.shape, n_ctx), r)
                assert np.array_equal(rv[..., 0].numpy(), e.valid) and int(rv.sum()) == e.kept, (p.name, r)


@DT
def test_c_oracle_on_the_probes(dtype):
    path = os.path.join(ROOT, "oracle", "_build", "liboracle_int.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    lib = C.CDLL(path)
    for p in probes(dtype):
        flat = np.ascontiguousarray(p.bits.reshape(-1))
        for r in p.ratios:
            e = sp.expect_threshold(p.bits, r, dtype)
            valid, thres = np.zeros(flat.size, dtype=np.uint8), C.c_double(0)
            assert lib.orc_threshold(flat.ctypes.data_as(C.c_void_p), C.c_int64(flat.size), C.c_double(r), int(dtype == sp.BF16),
                                     valid.ctypes.data_as(C.c_void_p), C.byref(thres)) == 0
            assert np.array_equal(valid.astype(bool), e.valid.reshape(-1)), (p.name, r)
            assert sp.same_class(_thres_bits(thres.value, dtype), e.thres_bits, dtype), (p.name, r)


@DT
def test_reference_fixture_pins_counting_and_oracle(dtype):
    """what the reference's own _threshold / _threshold_uniform returned on the exhaustive and degenerate probes (oracle/gen_golden.py:
    gen_select_specials): the probes are rebuilt from their seed and must be the recorded patterns"""
    g = load_golden("g16_select_specials.npz")
    seen = 0
    for p in sp.fixture_probes(dtype):
        assert np.array_equal(g[f"{p.name}/bits"], p.bits), p.name
        score = p.score
        for r in p.ratios:
            want = np.unpackbits(g[sp.fixture_key(p, "valid", r)])[:p.bits.size].astype(bool).reshape(p.bits.shape)
            tb = int(g[sp.fixture_key(p, "thres", r)][0])
            e = sp.expect_threshold(p.bits, r, dtype)
            ov, ot = orc.threshold(score, r)
            assert np.array_equal(e.valid, want) and np.array_equal(ov.numpy(), want), (p.name, r)
            assert sp.same_class(tb, e.thres_bits, dtype) and sp.same_class(tb, _thres_bits(ot, dtype), dtype), (p.name, r)
            seen += 1
        for k in p.ks:
            if 0 < k < p.bits.shape[-1]:
                want = np.unpackbits(g[sp.fixture_key(p, "topk", k)])[:p.bits.size].astype(bool).reshape(p.bits.shape)
                sp.check_topk_contract(f"{p.name}/k{k}", p.bits, sp.expect_topk(p.bits, k, dtype), want, k, dtype)
                seen += 1
    assert seen > 300


def test_twelve_patterns_of_the_issue():
    """the vector on which the divergence was found: the reference against the key as it was (a sign-bit NaN below -inf)"""
    b = np.array([0x3C00, 0xFE00, 0x3800, 0x7E00, 0x7C00, 0xFC00, 0x0001, 0x8001, 0x0000, 0x8000, 0xFE01, 0x3400], np.uint16).reshape(1, -1)
    for ratio, kept_ref, kept_old in ((0.3, 0, 1), (0.5, 2, 4), (0.9, 5, 8)):
        e = sp.expect_threshold(b, ratio, sp.F16)
        assert e.kept == kept_ref == int(sp.ref_threshold(sp.to_tensor(b, sp.F16), ratio)[0].sum())
        assert int(sp.radix_threshold(b, ratio, sp.F16, key=sp.order_key_sign_only)[1].sum()) == kept_old
        assert int(sp.radix_threshold(b, ratio, sp.F16)[1].sum()) == kept_ref


@DT
def test_fault_audit(dtype):
    """every fault must move the expectation of at least one probe - a condition, not a measurement"""
    caught = {name: [] for name in sp.MUTANTS}
    for p in probes(dtype):
        if p.bits.size > 20000 and "once" in p.name:
            rows = p.bits[:8]                                # (the top-k faults need a few rows only)
        else:
            rows = p.bits
        for name, (thr_kw, topk_kw) in sp.MUTANTS.items():
            if len(caught[name]) >= 3:
                continue
            hit = False
            if thr_kw is not None:
                for r in p.ratios:
                    e = sp.expect_threshold(p.bits, r, dtype)
                    tb, v = sp.radix_threshold(p.bits, r, dtype, **thr_kw)
                    if not np.array_equal(v, e.valid) or not sp.same_class(tb, e.thres_bits, dtype):
                        hit = True
                        break
            if not hit and topk_kw is not None:
                for k in p.ks:
                    if 0 < k < rows.shape[-1] and not np.array_equal(sp.radix_topk(rows, k, dtype, **topk_kw), sp.expect_topk(rows, k, dtype)):
                        hit = True
                        break
            if hit:
                caught[name].append(p.name)
    print("\nFAULT AUDIT", sp.tag(dtype))
    for name, where in caught.items():
        print(f"  {name:<42} caught by {where}")
    assert all(caught.values()), [n for n, w in caught.items() if not w]
    # fault 6 separately in both of its forms: +-0 and NaN payloads as distinct ties
    z = np.array([[0x8000, 0x0000, 0x8000, 0x0000, 0x3C00]], np.uint16)
    assert not np.array_equal(sp.radix_topk(z, 2, dtype, key=sp.order_key), sp.expect_topk(z, 2, dtype))
    inf = sp.INF[dtype]
    q = np.array([[inf + 1, inf + 2, 0x7FFF, 0x3C00]], np.uint16)
    assert not np.array_equal(sp.radix_topk(q, 1, dtype, key=sp.order_key), sp.expect_topk(q, 1, dtype))
    # and each threshold-side fault alone on the top-k side where it applies
    st = next(p for p in probes(dtype) if p.name.startswith("strata"))
    for name in ("1 sign-bit NaN ordered lowest", "4 rank - 1", "8 low-bin search ascending"):
        kw = sp.MUTANTS[name][1]
        assert any(not np.array_equal(sp.radix_topk(st.bits, k, dtype, **kw), sp.expect_topk(st.bits, k, dtype)) for k in st.ks), name
