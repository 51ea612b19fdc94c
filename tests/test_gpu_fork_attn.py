"""GPU: forked decode attention (kvz_fork_attn_append, kvz_attn_merge_lse) - exact probes (bit equality, tests/fork_probes.py),
oracle parity on random data, the first step of a branch, and B = 1 against the existing single-query path."""
import contextlib
import types

import pytest
import torch

import attn_probes as ap
import fork_probes as fp
import kvzip_oracle as orc
from conftest import check_attn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
# ragged shared lengths: a head with only its sink rows, a head long enough for several key ranges, edges of the 32-key wave tiles
LENS = [5, 3000, 129, 700]
ITEMS = 16     # attn_items knob of the exact cases: chunks of 256 keys, so the 3000-key head is cut into 12 ranges


def _ops():
    from kvzip_amd import ops
    return ops


@contextlib.contextmanager
def knob(name, val):
    lib = _ops()._lib.load()
    prev = lib.kvz_debug_set_tunable(name.encode(), int(val))
    try:
        yield
    finally:
        lib.kvz_debug_set_tunable(name.encode(), prev)


def _run(c, meta=True, dev_arrays=True):
    """One kvz_fork_attn_append call on the case's tensors -> (out, tail_k, tail_v, k, v) as the device holds them afterwards."""
    ops = _ops()
    q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    tk, tv = c.tail_k.to(DEV), c.tail_v.to(DEV)
    Hkv = len(c.lens)
    base = [n - c.k_len_offset for n in c.lens]
    ks = torch.tensor(c.starts, dtype=torch.int32, device=DEV) if dev_arrays else None
    kl = torch.tensor(base, dtype=torch.int32, device=DEV) if dev_arrays else None
    mh = ops._meta_host(c.starts, base, Hkv) if meta else None
    # the new rows arrive as the model produces them: K contiguous, V a strided view of the projection output
    kn = c.k_new.to(DEV)
    vn = c.v_new.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    out = ops.fork_attn_append(q, k, v, ks, kl, c.k_len_offset, tk, tv, c.tail_len, kn, vn, softmax_scale=c.scale, meta_host=mh)
    torch.cuda.synchronize()
    return out.cpu(), tk.cpu(), tv.cpu(), k.cpu(), v.cpu()


def _check_exact(name, c, **kw):
    out, tk, tv, k, v = _run(c, **kw)
    want = fp.expected_out(c)
    same, n = ap.bits_equal(out, want)
    print(f"\nFORK {name}: {n} of {want.numel()} outputs differ; worst {int(ap.steps(out, want).max())} steps")
    assert same, (name, n, int(ap.steps(out, want).max()))
    etk, etv = fp.expected_tails(c)
    assert ap.bits_equal(tk, etk)[0] and ap.bits_equal(tv, etv)[0], (name, "tails: only the new rows of active branches may change")
    assert ap.bits_equal(k, c.k)[0] and ap.bits_equal(v, c.v)[0], (name, "the shared cache was written")


def _tail_lens(B, cap, inactive=None):
    """tail_len in {0, 1, 37, cap - 1} mixed within one call, one branch inactive."""
    vals = [0, 1, 37, cap - 1]
    tl = [vals[b % 4] for b in range(B)]
    if inactive is not None and B > 1:
        tl[inactive % B] = -1
    return tl


GEOMS = [(7, 1, 128), (7, 2, 128), (7, 3, 128), (7, 9, 128), (4, 5, 128), (4, 16, 128), (2, 3, 64), (2, 16, 64)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,B,D", GEOMS)
def test_uniform_probe_exact(G, B, D, dtype):
    cap = 64
    with knob("attn_items", ITEMS):
        target = fp.fork_items(ITEMS, B, len(LENS), G)
        c = fp.uniform_case(LENS, B, G, D, dtype, _tail_lens(B, cap, inactive=B - 2), cap, items=(target,), seed=B)
        _check_exact(f"uniform G{G} B{B} D{D} {dtype}", c)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,B,D", GEOMS)
def test_weighted_probe_exact(G, B, D, dtype):
    cap = 64
    with knob("attn_items", ITEMS):
        c = fp.weighted_case(LENS, B, G, D, dtype, _tail_lens(B, cap, inactive=1), cap, seed=B)
        _check_exact(f"weighted G{G} B{B} D{D} {dtype}", c)


BOUNDARY_KEYS = {128: (8064, 8192), 64: (16256, 16384)}     # shared keys of the long head: 8 * 1024 / D - 1 key ranges of 128 keys, and one more


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (4, 64)])
def test_combine_at_the_boundary_between_its_two_paths(G, D, dtype):
    """The combine holds up to 8 partials per thread in registers (8 * 1024 / D per row) and takes its general path beyond.  With
    attn_items = 1024 a key range is its 128-key minimum, so a head of 8064 shared keys (D = 128; 16256 at D = 64) has, with the
    branch's tail, the last partial count of the fast path and a head of one range more the first of the general path.  The heads beside
    it have 1 and 0 keys (1 and 1 in the weighted case, which needs a key in every shared segment).  B = 2; a second call with branch 1
    inactive.  Split edges marked; both probe families."""
    B, cap = 2, 64
    with knob("attn_items", 1024):
        target = fp.fork_items(1024, B, 3, G)
        for n, partials in zip(BOUNDARY_KEYS[D], (8 * 1024 // D, 8 * 1024 // D + 1)):
            assert ap.decode_chunk([n, 1, 1], target) == 128 and n % 128 == 0 and n // 128 + 1 == partials
            for tl in ([37, 0], [37, -1]):
                _check_exact(f"uniform boundary {n} keys D{D} {dtype} tails {tl}",
                             fp.uniform_case([n, 1, 0], B, G, D, dtype, tl, cap, items=(target,), seed=n))
                _check_exact(f"weighted boundary {n} keys D{D} {dtype} tails {tl}",
                             fp.weighted_case([n, 1, 1], B, G, D, dtype, tl, cap, seed=n))


@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_offset_metadata_forms_and_default_items(kind):
    """A non-zero k_len_offset (rows a multi-turn update appended before the fork), head segments by value and / or as device arrays,
    the default work-item count, and a tail longer than one round of wave tiles."""
    cap = 600
    make = fp.uniform_case if kind == "uniform" else fp.weighted_case
    tl = [599, 0, -1, 300, 37]
    for meta, dev_arrays in ((True, True), (False, True), (True, False)):
        c = make(LENS, 5, 7, 128, torch.float16, tl, cap, k_len_offset=3, seed=7)
        _check_exact(f"{kind} offset 3 meta {meta} device arrays {dev_arrays}", c, meta=meta, dev_arrays=dev_arrays)
    with knob("attn_items", 3):     # fewer items than heads: every head is one range
        _check_exact(f"{kind} items 3", make(LENS, 2, 7, 128, torch.bfloat16, [1, 37], 64, seed=8))


def test_one_branch_of_64_rows():
    """B = 1, G = 64: four row tiles of ONE branch, the tail item is two blocks."""
    with knob("attn_items", ITEMS):
        _check_exact("uniform G64 B1", fp.uniform_case([5, 700], 1, 64, 64, torch.float16, [37], 64, seed=3))
        _check_exact("weighted G64 B1", fp.weighted_case([5, 700], 1, 64, 64, torch.float16, [37], 64, seed=3))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,B,D", [(7, 2, 128), (7, 9, 128), (4, 16, 128), (2, 5, 64)])
def test_oracle_parity_random(G, B, D, dtype):
    cap = 64
    c = fp.random_case([5, 3000, 129, 20000], B, G, D, dtype, _tail_lens(B, cap, inactive=0 if B > 2 else None), cap, k_len_offset=2, seed=B)
    out, tk, tv, k, v = _run(c)
    etk, etv = fp.expected_tails(c)
    assert ap.bits_equal(tk, etk)[0] and ap.bits_equal(tv, etv)[0] and ap.bits_equal(k, c.k)[0] and ap.bits_equal(v, c.v)[0]
    Hkv = len(c.lens)
    for b in range(B):
        if c.tail_len[b] < 0:
            assert bool((out[b] == 0).all())
            continue
        kk, vv, starts, lens = fp.concat_for_oracle(c, b)
        want = orc.varlen_attn(c.q[b].reshape(Hkv, G, D), kk, vv, starts, lens, 1)
        check_attn(f"fork/random/G{G}B{B}D{D}/{dtype}/b{b}", out[b].reshape(Hkv, G, D), want, TOL[dtype], ulp_of=dtype)


def _evict_cache(lens, G, D, dtype, slack=64, seed=0):
    """A pruned slack-layout EvictCache of one layer with the given head lengths (all rows kept: ratio 1 of ragged dense lengths is
    not expressible, so the score decides: head h keeps lens[h] - sink of N context rows)."""
    from kvzip_amd.kvcache import EvictCache
    Hkv, sink, N = len(lens), 4, max(lens)
    cfg = types.SimpleNamespace(num_hidden_layers=1, num_attention_heads=Hkv * G, num_key_value_heads=Hkv)
    g = torch.Generator().manual_seed(seed)
    kv = EvictCache(cfg, (sink, sink + N), device=DEV, dtype=dtype, slack=slack, verbose=False)
    kv.update(torch.randn(1, Hkv, sink + N, D, generator=g).to(dtype).to(DEV), torch.randn(1, Hkv, sink + N, D, generator=g).to(dtype).to(DEV), 0)
    score = torch.zeros(1, Hkv, N)
    for h, n in enumerate(lens):
        score[0, h, torch.randperm(N, generator=g)[:n - sink]] = 1.0
    kv.score = [score.to(dtype).to(DEV)]
    kept = sum(n - sink for n in lens)
    kv.prune((kept + 1.5) / (Hkv * N))   # threshold = a zero score: exactly the ones are kept
    assert kv.info["len_k_host"][0] == list(lens)
    return kv


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_one_branch_equals_the_existing_path(dtype):
    """fork(1) + decode steps vs EvictCache.update_attend on a cache with the same rows."""
    G, D, lens = 7, 128, [4, 2500, 131, 640]
    a, b = _evict_cache(lens, G, D, dtype), _evict_cache(lens, G, D, dtype)
    seg = a.info["seg_start"][0].tolist()
    assert seg == b.info["seg_start"][0].tolist()
    for h, n in enumerate(lens):    # (the slack rows behind the segments are uninitialised memory)
        assert torch.equal(a.key_cache[0][seg[h]:seg[h] + n], b.key_cache[0][seg[h]:seg[h] + n])
    before_k, before_v = a.key_cache[0].clone(), a.value_cache[0].clone()
    fork = a.fork(1, tail_capacity=2)      # (outgrown at the third step: the tail is re-allocated)
    g = torch.Generator().manual_seed(5)
    for step in range(4):
        q = torch.randn(1, len(lens) * G, 1, D, generator=g).to(dtype).to(DEV)
        k = torch.randn(1, len(lens), 1, D, generator=g).to(dtype).to(DEV)
        v = torch.randn(1, len(lens), 1, D, generator=g).to(dtype).to(DEV)
        got = fork.update_attend(q, k, v, 0)
        want = b.update_attend(q, k, v, 0)
        check_attn(f"fork/B1-vs-update_attend/{dtype}/step{step}", got.reshape(want.shape), want, TOL[dtype], ulp_of=dtype)
    assert fork.tail_len[0] == [4] and fork.tail_k[0].shape[2] >= 4
    assert a.info["offset"] == [0] and a.get_seq_length() == b.get_seq_length() - 4
    assert ap.bits_equal(a.key_cache[0], before_k)[0] and ap.bits_equal(a.value_cache[0], before_v)[0]   # slack rows included


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("q_len", [2, 11, 70])
def test_first_step_matches_oracle(q_len, dtype):
    """A branch's query: two kvz_flash_fwd calls (shared segments unmasked, tail causal) merged by their LSEs, against the oracle on
    the explicit concatenation with the bottom-right causal mask; then one decode step of both branches on top."""
    G, D, lens = 7, 128, [4, 2500, 131, 640]
    Hkv = len(lens)
    kv = _evict_cache(lens, G, D, dtype)
    fork = kv.fork(2, tail_capacity=8)
    g = torch.Generator().manual_seed(q_len)
    rows = {}
    for b, n in ((1, q_len), (0, 3)):
        q = torch.randn(1, Hkv * G, n, D, generator=g).to(dtype).to(DEV)
        k = torch.randn(1, Hkv, n, D, generator=g).to(dtype).to(DEV)
        v = torch.randn(1, Hkv, n, D, generator=g).to(dtype).to(DEV)
        fork.select_branch(b)
        got = fork.first_step(q, k, v, 0).cpu()                       # [Hkv, n, G, D]
        rows[b] = (k.cpu(), v.cpu())
        seg = kv.info["seg_start"][0].tolist()
        ks, vs, starts, ln, acc = [], [], [], [], 0
        for h in range(Hkv):
            ks += [kv.key_cache[0][seg[h]:seg[h] + lens[h]].cpu(), k[0, h].cpu()]
            vs += [kv.value_cache[0][seg[h]:seg[h] + lens[h]].cpu(), v[0, h].cpu()]
            starts.append(acc); ln.append(lens[h] + n); acc += lens[h] + n
        qo = q[0].cpu().view(Hkv, G, n, D).transpose(1, 2).reshape(Hkv * n, G, D)
        want = orc.varlen_attn(qo, torch.cat(ks), torch.cat(vs), starts, ln, n, causal=True)
        check_attn(f"fork/first-step/q{n}/{dtype}/b{b}", got.reshape(Hkv * n, G, D), want, TOL[dtype], ulp_of=dtype)
    assert fork.tail_len[0] == [3, q_len]
    for b in (0, 1):
        t = fork.tail_len[0][b]
        assert torch.equal(fork.tail_k[0][b, :, :t].cpu(), rows[b][0][0]) and torch.equal(fork.tail_v[0][b, :, :t].cpu(), rows[b][1][0])
    # a decode step of both branches over shared ++ their tails
    q = torch.randn(2, Hkv * G, 1, D, generator=g).to(dtype).to(DEV)
    k = torch.randn(2, Hkv, 1, D, generator=g).to(dtype).to(DEV)
    v = torch.randn(2, Hkv, 1, D, generator=g).to(dtype).to(DEV)
    got = fork.update_attend(q, k, v, 0).cpu()
    seg = kv.info["seg_start"][0].tolist()
    for b in (0, 1):
        ks, vs, starts, ln, acc = [], [], [], [], 0
        for h in range(Hkv):
            ks += [kv.key_cache[0][seg[h]:seg[h] + lens[h]].cpu(), rows[b][0][0, h], k[b, h].cpu()]
            vs += [kv.value_cache[0][seg[h]:seg[h] + lens[h]].cpu(), rows[b][1][0, h], v[b, h].cpu()]
            n = lens[h] + rows[b][0].shape[2] + 1
            starts.append(acc); ln.append(n); acc += n
        want = orc.varlen_attn(q[b].cpu().view(Hkv, G, D), torch.cat(ks), torch.cat(vs), starts, ln, 1)
        check_attn(f"fork/decode-after-first-step/{dtype}/b{b}", got[b].reshape(Hkv, G, D), want, TOL[dtype], ulp_of=dtype)


def test_merge_lse_rows_without_keys():
    """Rows whose both LSEs are -inf give zero; a side with -inf is ignored whatever it holds."""
    ops = _ops()
    o1 = torch.randn(6, 128).half().to(DEV)
    o2 = torch.randn(6, 128).half().to(DEV)
    o2[1] = float("nan")
    inf = float("-inf")
    l1 = torch.tensor([0.0, 1.0, inf, inf, 2.0, -3.0], device=DEV)
    l2 = torch.tensor([0.0, inf, 1.0, inf, 2.0 + 0.6931471805599453, 5.0], device=DEV)
    out = ops.attn_merge_lse(o1, l1, o2, l2).cpu().float()
    a, b = o1.cpu().float(), o2.cpu().float()
    assert torch.equal(out[1], a[1]) and torch.equal(out[2], b[2]) and bool((out[3] == 0).all())
    assert (out[0] - (a[0] + b[0]) / 2).abs().max() <= 2e-3
    assert (out[4] - (a[4] + 2 * b[4]) / 3).abs().max() <= 2e-3


def test_stale_fork_raises():
    """A fork outlived by a re-laid-out base raises instead of reading moved rows."""
    from kvzip_amd.ops import KvzError
    G, D, lens = 7, 128, [4, 300, 131, 64]
    kv = _evict_cache(lens, G, D, torch.float16, slack=4)
    fork = kv.fork(2)
    q = torch.randn(2, 4 * G, 1, D).half().to(DEV)
    k = torch.randn(2, 4, 1, D).half().to(DEV)
    fork.update_attend(q, k, k, 0)
    kv._grow_slack(16)
    with pytest.raises(KvzError, match="re-laid out"):
        fork.update_attend(q, k, k, 0)
    with pytest.raises(KvzError, match="re-laid out"):
        fork.first_step(q[:1], k[:1], k[:1], 0)
    fork2 = kv.fork(2)                     # a new fork of the new layout works
    fork2.update_attend(q, k, k, 0)
    with pytest.raises(KvzError):
        kv.fork(10)                        # 10 x 7 > 64 query rows per KV head
