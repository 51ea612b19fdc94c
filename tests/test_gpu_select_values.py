"""GPU: the selection kernels over every 16-bit score pattern (tests/select_probes.py) - NaNs of both signs and all payloads, infinities,
subnormals, both zeros, multisets inside one radix bin, ranks on bin edges, all-equal and tiny inputs, poisoned heads - through
ops.select_threshold (plain and on the histogram of kvz_score_finalize_log_hist), ops.select_topk_rows, ops.select_heads, ops.rowmax
and EvictCache.prune.

Everything is exact, there are no tolerances: masks, kept counts and row counts equal what the probes expect by counting (which
tests/test_select_probes.py pins to the reference's expressions, the oracles and tests/golden/g16_select_specials.npz), and the
threshold is the expected NUMBER: the same bits, or a NaN where a NaN is expected, or a zero where a zero is expected (which NaN payload,
which zero the reference's sort leaves at the rank is its unspecified order among equal values)."""
import types

import numpy as np
import pytest
import torch

import kvzip_oracle as orc
import select_probes as sp
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = pytest.mark.parametrize("dtype", sp.DTYPES, ids=["f16", "bf16"])
FAMILIES = ["exhaustive", "bin-edge", "degenerate", "poisoned"]
_cache = {}


def ops():
    from kvzip_amd import ops as o
    return o


def probes(dtype, family=None):
    if dtype not in _cache:
        _cache[dtype] = sp.all_probes(dtype)
    return [p for p in _cache[dtype] if family is None or p.family == family]


def _thres_ok(t: torch.Tensor, want_bits: int, dtype) -> bool:
    return sp.same_class(sp.f32_to_bits(float(t.item()), dtype), want_bits, dtype)


def _check_threshold(p, ratio, got, fails, how):
    v, t, k, rc = got
    e = sp.expect_threshold(p.bits, ratio, p.dtype)
    ok = (np.array_equal(v.cpu().numpy().reshape(p.bits.shape), e.valid) and _thres_ok(t, e.thres_bits, p.dtype)
          and int(k.item()) == e.kept and np.array_equal(rc.cpu().numpy(), e.row_counts))
    if not ok:
        fails.append((p.name, ratio, how, float(t.item()), hex(e.thres_bits), int(k.item()), e.kept))


def _prehist(o, bits_dev, dtype):
    """the patterns through kvz_score_finalize_log_hist: a log buffer that holds the fill pattern only (nothing scored) leaves `out`
    as it stands - the patterns are the stale values - and histograms them.  -> (scores, workspace)"""
    lib = o._lib.load()
    n = bits_dev.numel()
    log = torch.empty(n, dtype=torch.int32, device=DEV)
    out = bits_dev.clone()
    ws = o.select_workspace(DEV)
    st = o._stream(out)
    o.check(lib.kvz_score_log_fill(log.data_ptr(), n, st), "kvz_score_log_fill")
    o.check(lib.kvz_score_finalize_log_hist(log.data_ptr(), n, out.data_ptr(), o._dtype_code(dtype), ws.data_ptr(), ws.numel(), st),
            "kvz_score_finalize_log_hist")
    return out, ws


@DT
@pytest.mark.parametrize("family", FAMILIES)
def test_select_threshold_plain_and_prehist(dtype, family):
    o = ops()
    fails = []
    for p in probes(dtype, family):
        score = p.score.to(DEV)
        row_len = p.bits.shape[-1]
        for ratio in p.ratios:
            _check_threshold(p, ratio, o.select_threshold(score, ratio, row_len=row_len), fails, "plain")
            out, ws = _prehist(o, score, dtype)
            assert torch.equal(out.view(torch.int16), score.view(torch.int16)), p.name
            _check_threshold(p, ratio, o.select_threshold(out, ratio, row_len=row_len, prehist=ws), fails, "prehist")
    assert not fails, (len(fails), fails[:12])


@DT
def test_reference_fixture_on_the_kernels(dtype):
    """the masks and thresholds the REFERENCE returned (tests/golden/g16_select_specials.npz), straight against the kernels"""
    o = ops()
    g = load_golden("g16_select_specials.npz")
    fails = []
    for p in sp.fixture_probes(dtype):
        score = p.score.to(DEV)
        for ratio in p.ratios:
            v, t, k, rc = o.select_threshold(score, ratio, row_len=p.bits.shape[-1])
            want = np.unpackbits(g[sp.fixture_key(p, "valid", ratio)])[:p.bits.size].astype(bool).reshape(p.bits.shape)
            tb = int(g[sp.fixture_key(p, "thres", ratio)][0])
            if not (np.array_equal(v.cpu().numpy(), want) and _thres_ok(t, tb, dtype) and int(k.item()) == int(want.sum())):
                fails.append((p.name, ratio, float(t.item()), hex(tb)))
        for kk in p.ks:
            if 0 < kk < p.bits.shape[-1]:
                v, _ = o.select_topk_rows(score, kk)
                want = np.unpackbits(g[sp.fixture_key(p, "topk", kk)])[:p.bits.size].astype(bool).reshape(p.bits.shape)
                sp.check_topk_contract(f"{p.name}/k{kk}", p.bits, v.cpu().numpy(), want, kk, dtype)
    assert not fails, (len(fails), fails[:12])


@DT
def test_prehist_with_real_log_entries_and_the_nan_code(dtype):
    """a log buffer with real entries (log-scores), entries of 0 (the code of a NaN score) and never-scored entries whose stale values
    are arbitrary patterns: the finalize + histogram launch and the prehist selection against the counting on the scores it wrote"""
    o = ops()
    lib = o._lib.load()
    fails = []
    for rows, row_len in ((7, 1003), (4, 4096), (1, 13)):
        n = rows * row_len
        g = torch.Generator().manual_seed(n)
        logs = -(torch.rand(n, generator=g) * 9.0)
        log_bits = logs.view(torch.int32).clone()
        kind = torch.rand(n, generator=g)
        log_bits[kind < 0.15] = 0                                                            # NaN code
        log_bits[kind > 0.6] = torch.tensor(0xFF800000 - (1 << 32), dtype=torch.int32)       # never scored
        stale = torch.from_numpy(np.random.default_rng(n).integers(0, 65536, n).astype(np.uint16).view(np.int16)).view(dtype)
        log_d, out, ws = log_bits.to(DEV), stale.to(DEV), o.select_workspace(DEV)
        st = o._stream(out)
        for ratio in (0.0, 0.05, 0.14, 0.16, 0.3, 0.45, 0.6, 0.9, 0.999):
            out.copy_(stale)
            o.check(lib.kvz_score_finalize_log_hist(log_d.data_ptr(), n, out.data_ptr(), o._dtype_code(dtype), ws.data_ptr(), ws.numel(), st), "hist")
            bits = out.cpu().view(torch.int16).numpy().view(np.uint16).reshape(rows, row_len)
            flat = bits.reshape(-1)
            assert sp.is_nan(flat[(kind < 0.15).numpy()], dtype).all()
            assert np.array_equal(flat[(kind > 0.6).numpy()], stale.view(torch.int16).numpy().view(np.uint16)[(kind > 0.6).numpy()])
            p = sp.Probe(f"mixed-log/{rows}x{row_len}/{sp.tag(dtype)}", dtype, bits, (ratio,))
            _check_threshold(p, ratio, o.select_threshold(out.view(rows, row_len), ratio, row_len=row_len, prehist=ws), fails, "prehist")
            _check_threshold(p, ratio, o.select_threshold(out.view(rows, row_len), ratio, row_len=row_len), fails, "plain")
    assert not fails, (len(fails), fails[:12])


@DT
def test_select_threshold_over_launch_geometries_on_edge_and_tail_probes(dtype):
    """sel_blocks x emit_blocks as tests/test_gpu_kernels.py::test_select_threshold_over_launch_geometries sweeps them, on the probes whose
    specials sit in the last n % 8 elements, at row ends and on bin edges"""
    o = ops()
    lib = o._lib.load()
    fails = []
    todo = [p for p in probes(dtype) if p.sweep]
    assert len(todo) >= 6
    for sb in (1, 2, 3, 7, 0, 1024):
        for eb in (1, 5, 0, 4096):
            prev_s = lib.kvz_debug_set_tunable(b"sel_blocks", sb)
            prev_e = lib.kvz_debug_set_tunable(b"emit_blocks", eb)
            try:
                for p in todo:
                    score = p.score.to(DEV)
                    for ratio in p.ratios[::3]:
                        _check_threshold(p, ratio, o.select_threshold(score, ratio, row_len=p.bits.shape[-1]), fails, f"plain sb{sb} eb{eb}")
                        out, ws = _prehist(o, score, dtype)
                        _check_threshold(p, ratio, o.select_threshold(out, ratio, row_len=p.bits.shape[-1], prehist=ws), fails,
                                         f"prehist sb{sb} eb{eb}")
            finally:
                lib.kvz_debug_set_tunable(b"sel_blocks", prev_s)
                lib.kvz_debug_set_tunable(b"emit_blocks", prev_e)
    assert not fails, (len(fails), fails[:12])


@DT
@pytest.mark.parametrize("family", FAMILIES)
def test_select_topk_rows(dtype, family):
    """exactly k per row, every value above the k-th largest AS A NUMBER, and of the entries equal to it the lowest indices - which is
    what the probes expect by counting, bit for bit (and the reference's kept multiset: tests/test_select_probes.py)"""
    o = ops()
    fails = []
    for p in probes(dtype, family):
        score = p.score.to(DEV)
        N = p.bits.shape[-1]
        for k in sorted(set(p.ks) | {0, N}):
            v, rc = o.select_topk_rows(score, k)
            e = sp.expect_topk(p.bits, k, dtype)
            if not (np.array_equal(v.cpu().numpy(), e) and bool((rc.cpu() == min(k, N)).all())):
                fails.append((p.name, k, int((v.cpu().numpy() != e).sum())))
    assert not fails, (len(fails), fails[:12])


@DT
@pytest.mark.parametrize("n_ctx", [1, 7, 131072])
def test_select_heads(dtype, n_ctx):
    o = ops()
    fails = []
    for p in probes(dtype):
        if p.bits.size > 4096:
            continue
        score = p.score
        for ratio in p.ratios + (0.05, 0.5):
            v, t, k, rc = o.select_heads(score.to(DEV), n_ctx, ratio)
            e = sp.expect_heads(p.bits, n_ctx, ratio, dtype)
            ov, ot = orc.threshold_heads(score, n_ctx, ratio)
            ok = (np.array_equal(v.cpu().numpy(), e.valid) and np.array_equal(v.cpu().numpy(), ov.numpy()) and _thres_ok(t, e.thres_bits, dtype)
                  and sp.same_class(sp.f32_to_bits(ot, dtype), e.thres_bits, dtype) and int(k.item()) == e.kept
                  and np.array_equal(rc.cpu().numpy(), e.row_counts))
            if not ok:
                fails.append((p.name, ratio, float(t.item()), hex(e.thres_bits), int(k.item()), e.kept))
    assert not fails, (len(fails), fails[:12])


@DT
def test_rowmax(dtype):
    """against torch.amax: a row with a NaN gives a NaN (any payload), otherwise the bits of the maximum; an all -inf row gives -inf, a
    row of -0 only gives -0 (of +0 and -0 mixed: a zero); row_len 1"""
    o = ops()
    inf = sp.INF[dtype]
    cases = [p.bits for p in probes(dtype) if p.bits.size <= 80000]
    cases += [np.full((3, 37), 0x8000 | inf, np.uint16), np.full((2, 1000), 0x8000, np.uint16), np.array([[0x8000, 0, 0x8000]], np.uint16),
              np.arange(65536, dtype=np.uint16).reshape(-1, 1), np.arange(65536, dtype=np.uint16).reshape(-1, 32)]
    for i, b in enumerate(cases):
        got = o.rowmax(sp.to_tensor(b, dtype).to(DEV)).cpu().view(torch.int16).numpy().view(np.uint16)
        want = torch.amax(sp.to_tensor(b, dtype), dim=-1).view(torch.int16).numpy().view(np.uint16)
        ck = sp.class_key(b, dtype).max(-1)                  # by counting: the highest value class of the row
        assert np.array_equal(sp.class_key(got, dtype), ck), i
        assert np.array_equal(sp.class_key(want, dtype), ck), i
        exact = (ck != sp.NAN_CLASS) & (ck != sp.ZERO_CLASS)   # (a NaN of any payload, either zero of a row whose maximum is zero)
        assert np.array_equal(got[exact], want[exact]) and np.array_equal(got[exact], sp.key_inv(ck[exact])), i
    assert int(o.rowmax(sp.to_tensor(np.full((1, 9), 0x8000, np.uint16), dtype).to(DEV)).view(torch.int16).item()) & 0xFFFF == 0x8000
    assert int(o.rowmax(sp.to_tensor(np.full((1, 9), 0x8000 | inf, np.uint16), dtype).to(DEV)).view(torch.int16).item()) & 0xFFFF == 0x8000 | inf


@DT
@pytest.mark.parametrize("ratio", [0.1, 0.4], ids=["nans-beyond-rank", "rank-beyond-nans"])
def test_prune_with_deferred_scores_and_a_poisoned_head(dtype, ratio):
    """EvictCache.prune on deferred scores (the histogram of the finalize launch feeds the selection) with a NaN in Q that poisons one
    KV head of one layer - 1/6 of all scores: at ratio 0.1 the rank lies inside the NaNs (NaN threshold, nothing kept: the fallback
    to the plain path must not raise), at 0.4 beyond them.  Mask, threshold and kept ratio against orc.threshold on the scores."""
    from kvzip_amd.kvcache import EvictCache
    L, H, Hkv, D, sink, N = 3, 8, 2, 128, 16, 512
    cfg = types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=H, num_key_value_heads=Hkv)
    g = torch.Generator(device=DEV).manual_seed(11)
    kv = EvictCache(cfg, (sink, sink + N), device=DEV, dtype=dtype, verbose=False)
    assert kv.score_deferred
    for l in range(L):
        k0 = torch.randn(1, Hkv, sink + N, D, generator=g, device=DEV).to(dtype)
        kv.update(k0, k0, l)
    kv.init_score()
    kv.start_idx, kv.end_idx = sink, sink + N
    seen = kv._seen_tokens
    for l in range(L):
        q = torch.randn(1, H, N + 9, D, generator=g, device=DEV).to(dtype)
        kr = torch.randn(1, Hkv, N + 9, D, generator=g, device=DEV).to(dtype)
        if l == 1:
            q[0, 5, 77, 3] = float("inf")                   # query head 5 -> KV head 1 of layer 1
        k_all, _ = kv.update(kr, kr, l)
        kv._get_score(q, k_all, l)
    kv.slice(seen)
    kv.start_idx, kv.get_score = sink, False
    thres, r_real = kv.prune(ratio)
    score = torch.stack([s.clone() for s in kv.score]).cpu()
    nan = score.isnan()
    assert bool(nan[1, 0, 1].all()) and int(nan.sum()) == N, "one KV head of one layer is poisoned, nothing else"
    nb = np.unique(score[nan].view(torch.int16).numpy().view(np.uint16))
    print(f"\nNaN patterns on the scoring path ({sp.tag(dtype)}):", [hex(int(x)) for x in nb])
    want_v, want_t = orc.threshold(score, ratio)
    valid = kv.valid.cpu().view(want_v.shape)
    assert torch.equal(valid, want_v), "the mask differs from the reference's"
    assert not bool((valid & ~want_v).any())
    assert (thres != thres and want_t != want_t) or thres == want_t, (thres, want_t)
    if ratio == 0.1:
        assert thres != thres and not bool(valid.any())
    else:
        assert thres == thres and 0 < int(valid.sum()) <= int(score.numel() * ratio) - 1 - N   # (the NaNs take N ranks and are never kept)
