"""GPU: batched decode over several independent pruned caches (kvz_multi_attn_append, kvcache.CacheBatch) - exact probes (bit
equality, tests/multi_probes.py), an inactive cache, the appended rows, oracle parity on random data, and the life cycle of a
CacheBatch against caches stepped alone."""
import contextlib
import types

import pytest
import torch

import attn_probes as ap
import kvzip_oracle as orc
import multi_probes as mp
from conftest import check_attn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}     # the bounds of test_gpu_fork_attn.py
# B = 3 caches of Hkv = 2 heads: a head of several key ranges beside a head of one wave tile, an EMPTY head (a dropped head of a
# head-level cache), edges of the 32-key wave tiles and of the 128-key chunk unit
LENS = [[3000, 37], [0, 129], [64, 255]]
OFFSETS = [0, 5, 1]
SLACK = 8


def _ops():
    from kvzip_amd import ops
    return ops


@contextlib.contextmanager
def knob(name, val):
    lib = _ops()._lib.load()
    if val is None:     # the default
        yield
        return
    prev = lib.kvz_debug_set_tunable(name.encode(), int(val))
    try:
        yield
    finally:
        lib.kvz_debug_set_tunable(name.encode(), prev)


def device_case(c):
    """The case's tensors on the device: (q, arena_k, arena_v, per-cache K views, per-cache V views, k_new, v_new).  The new rows arrive
    as the model produces them: K contiguous, V a strided view of the projection output."""
    ak, av = c.arena_k.to(DEV), c.arena_v.to(DEV)
    ks = [ak[r:r + n] for r, n in zip(c.row0, c.rows)]
    vs = [av[r:r + n] for r, n in zip(c.row0, c.rows)]
    kn = c.k_new.to(DEV)
    vn = c.v_new.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    return c.q.to(DEV), ak, av, ks, vs, kn, vn


def _run(c):
    """One kvz_multi_attn_append call -> (out, arena_k, arena_v) as the device holds them afterwards."""
    ops = _ops()
    q, ak, av, ks, vs, kn, vn = device_case(c)
    table = ops.MultiTable(ks, vs, c.starts, c.lens, c.slack)
    out = ops.multi_attn_append(q, table, c.offset, kn, vn, softmax_scale=c.scale)
    torch.cuda.synchronize()
    return out.cpu(), ak.cpu(), av.cpu()


def _check_exact(name, c):
    out, ak, av = _run(c)
    want = mp.expected_out(c)
    same, n = ap.bits_equal(out, want)
    print(f"\nMULTI {name}: {n} of {want.numel()} outputs differ; worst {int(ap.steps(out, want).max())} steps")
    assert same, (name, n, int(ap.steps(out, want).max()))
    ek, ev = mp.expected_arenas(c)
    assert ap.bits_equal(ak, ek)[0] and ap.bits_equal(av, ev)[0], (name, "only the new row of every live (cache, head) may change")
    return out


@pytest.mark.parametrize("items", [3, 16, None], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 4, 7, 20])
def test_probes_exact(G, D, dtype, items):
    """items 3: fewer items than segments, every segment is one range; 16: the 3000-key segment is cut into many ranges while the
    37-key one is one; default: one block per CU.  G = 20: two row tiles."""
    with knob("attn_items", items):
        target = mp.multi_items(items or 0, 6)
        _check_exact(f"uniform G{G} D{D} {dtype} items {items}", mp.uniform_case(LENS, OFFSETS, G, D, dtype, SLACK, items=(target,), seed=G))
        _check_exact(f"weighted G{G} D{D} {dtype} items {items}", mp.weighted_case(LENS, OFFSETS, G, D, dtype, SLACK, seed=G))


@pytest.mark.parametrize("items", [3, 16, None], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_inactive_cache(kind, items):
    """Cache 1 inactive (offset -1): its output rows are zero, its K,V are byte-identical to before (the whole arenas are compared),
    and the other two caches give what they give when all three are live."""
    G, D, dtype = 7, 128, torch.float16
    make = (lambda off: mp.uniform_case(LENS, off, G, D, dtype, SLACK, items=(mp.multi_items(items or 0, 6),), seed=3)) \
        if kind == "uniform" else (lambda off: mp.weighted_case(LENS, off, G, D, dtype, SLACK, seed=3))
    with knob("attn_items", items):
        live = _check_exact(f"{kind} all live", make(OFFSETS))
        c = make([0, -1, 1])
        out = _check_exact(f"{kind} cache 1 inactive", c)
    assert bool((out[1] == 0).all())
    assert ap.bits_equal(out[0], live[0])[0] and ap.bits_equal(out[2], live[2])[0]
    # nothing live at all: no work item, zeros
    with knob("attn_items", items):
        out = _check_exact(f"{kind} nothing live", make([-1, -1, -1]))
    assert bool((out == 0).all())


BOUNDARY_KEYS = {128: (8192, 8193), 64: (16384, 16385)}     # keys of the long segment: 8 * 1024 / D key ranges of 128 keys, and one more


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", [(7, 128), (4, 64)])
def test_combine_at_the_boundary_between_its_two_paths(G, D, dtype):
    """The combine holds up to 8 partials per thread in registers (8 * 1024 / D per row) and takes its general path beyond.  With
    attn_items = 1024 a key range is its 128-key minimum, so a segment of 8192 keys, the new row included (D = 128; 16384 at D = 64),
    has the last partial count of the fast path and a segment of one key more the first of the general path.  Two caches, the segments
    beside the long one of 1, 0 and 37 base rows; a second call with the second cache inactive.  Split edges marked; both families."""
    with knob("attn_items", 1024):
        for n, partials in zip(BOUNDARY_KEYS[D], (8 * 1024 // D, 8 * 1024 // D + 1)):
            lens = [[n - 1, 1], [0, 37]]
            for off in ([0, 0], [0, -1]):
                for c in (mp.uniform_case(lens, off, G, D, dtype, SLACK, items=(1024,), seed=n),
                          mp.weighted_case(lens, off, G, D, dtype, SLACK, seed=n)):
                    seg = c.segment_lengths()
                    assert seg[0] == n and ap.decode_chunk(seg, mp.multi_items(1024, 4)) == 128 and -(-n // 128) == partials
                    out = _check_exact(f"{c.kind} boundary {n} keys D{D} {dtype} offsets {off}", c)
                    assert off[1] >= 0 or bool((out[1] == 0).all())


def _check_oracle(name, c):
    out, ak, av = _run(c)
    ek, ev = mp.expected_arenas(c)
    assert ap.bits_equal(ak, ek)[0] and ap.bits_equal(av, ev)[0], (name, "appended rows")
    B, Hkv, G, D = c.q.shape
    for b in range(B):
        if c.offset[b] < 0:
            assert bool((out[b] == 0).all())
            continue
        kk, vv, starts, lens = mp.concat_for_oracle(c, b)
        want = orc.varlen_attn(c.q[b].reshape(Hkv, G, D), kk, vv, starts, lens, 1)
        check_attn(f"multi/random/{name}/b{b}", out[b].reshape(Hkv, G, D), want, TOL[c.dtype], ulp_of=c.dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_oracle_parity_random(dtype):
    g = torch.Generator().manual_seed(11)
    # B = 1; B = 4 with very different caches (and one inactive); the limit B * Hkv = 128 with lengths <= 200
    _check_oracle(f"B1/{dtype}", mp.random_case([[5, 3000, 129, 700]], [2], 7, 128, dtype, seed=1))
    _check_oracle(f"B4/{dtype}", mp.random_case([[2500, 31], [0, 640], [129, 128], [1, 77]], [0, 3, -1, 7], 7, 128, dtype, seed=2))
    lens = torch.randint(0, 201, (16, 8), generator=g).tolist()
    offs = torch.randint(0, 6, (16,), generator=g).tolist()
    _check_oracle(f"B16xHkv8/{dtype}", mp.random_case(lens, offs, 4, 64, dtype, seed=3))
    with knob("attn_items", 16):
        _check_oracle(f"B16xHkv8/items16/{dtype}", mp.random_case(lens, offs, 20, 128, dtype, seed=4))


# ---- CacheBatch life cycle ----------------------------------------------------------------------------------------------------------
L, HKV, G_, D_ = 2, 2, 4, 64


def _evict_cache(N, seed, dtype=torch.float16, slack=16, ratio=0.5):
    """A pruned slack-layout EvictCache of L layers over N context tokens with random scores."""
    from kvzip_amd.kvcache import EvictCache
    sink = 4
    cfg = types.SimpleNamespace(num_hidden_layers=L, num_attention_heads=HKV * G_, num_key_value_heads=HKV)
    g = torch.Generator().manual_seed(seed)
    kv = EvictCache(cfg, (sink, sink + N), device=DEV, dtype=dtype, slack=slack, verbose=False)
    for l in range(L):
        kv.update(torch.randn(1, HKV, sink + N, D_, generator=g).to(dtype).to(DEV), torch.randn(1, HKV, sink + N, D_, generator=g).to(dtype).to(DEV), l)
    kv.score = [torch.rand(1, HKV, N, generator=g).to(dtype).to(DEV) for _ in range(L)]
    kv.prune(ratio)
    return kv


def _segments(kv, l):
    """per head (K, V) of the rows layer l holds, appended ones included (CPU)"""
    seg, lens, off = kv.info["seg_start"][l].tolist(), kv.info["len_k_host"][l], kv.info["offset"][l]
    return [(kv.key_cache[l][seg[h]:seg[h] + lens[h] + off].cpu(), kv.value_cache[l][seg[h]:seg[h] + lens[h] + off].cpu()) for h in range(HKV)]


def _step_inputs(g, B, dtype=torch.float16):
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).to(DEV)  # noqa: E731
    return [(mk(B, HKV * G_, 1, D_), mk(B, HKV, 1, D_), mk(B, HKV, 1, D_)) for _ in range(L)]


def _oracle_step(kvs, before, inputs, outs, name):
    """Every live member's output of a batched step against the oracle on (the rows the member held before) ++ (its new row)."""
    for l in range(L):
        q, k, v = inputs[l]
        for b, kv in enumerate(kvs):
            ks, vs, starts, lens, acc = [], [], [], [], 0
            for h in range(HKV):
                kh = torch.cat([before[b][l][h][0], k[b, h].cpu()])
                vh = torch.cat([before[b][l][h][1], v[b, h].cpu()])
                ks.append(kh); vs.append(vh); starts.append(acc); lens.append(kh.shape[0]); acc += kh.shape[0]
            want = orc.varlen_attn(q[b].cpu().view(HKV, G_, D_), torch.cat(ks), torch.cat(vs), starts, lens, 1)
            check_attn(f"multi/batch/{name}/l{l}/b{b}", outs[l][b].cpu(), want, TOL[torch.float16], ulp_of=torch.float16)


def test_cache_batch_life_cycle():
    from kvzip_amd.kvcache import CacheBatch
    kvs = [_evict_cache(300, 1), _evict_cache(417, 2)]
    alone = [_evict_cache(300, 1), _evict_cache(417, 2)]          # the same two caches again, stepped alone
    for a, b in zip(kvs, alone):
        assert a.info["len_k_host"] == b.info["len_k_host"] and a.get_seq_length() == b.get_seq_length()
    assert kvs[0].info["len_k_host"] != kvs[1].info["len_k_host"]
    g = torch.Generator().manual_seed(7)
    for _ in range(2):             # member 1 starts two rows ahead: the offsets differ between the members
        for l, (q, k, v) in enumerate(_step_inputs(g, 1)):
            kvs[1].update_attend(q, k, v, l), alone[1].update_attend(q, k, v, l)
    batch = CacheBatch(kvs)
    assert batch.layout == "multi" and batch.n_caches == 2
    for step in range(3):
        inputs = _step_inputs(g, 2)
        for l in range(L):
            q, k, v = inputs[l]
            got = batch.update_attend(q, k, v, l)
            assert got.shape == (2, HKV, G_, D_)
            for b in range(2):
                want = alone[b].update_attend(q[b:b + 1], k[b:b + 1], v[b:b + 1], l)
                check_attn(f"multi/batch-vs-alone/step{step}/l{l}/b{b}", got[b], want, TOL[torch.float16], ulp_of=torch.float16)
        for a, b in zip(kvs, alone):
            assert a.info["offset"] == b.info["offset"] and a._seen_tokens == b._seen_tokens and a._mem() == b._mem()
            for l in range(L):
                for (ka, va), (kb, vb) in zip(_segments(a, l), _segments(b, l)):
                    assert ap.bits_equal(ka, kb)[0] and ap.bits_equal(va, vb)[0], ("rows", step, l)
    assert kvs[0].info["offset"] == [3, 3] and kvs[1].info["offset"] == [5, 5]
    # slice one member, tighten the other (its flat cache moves: the batch rebuilds its table), step the batch again
    kvs[0].slice(kvs[0].get_seq_length() - 3)
    assert kvs[0].info["offset"] == [0, 0]
    epoch = kvs[1]._layout_epoch
    kvs[1].tighten(0.3)
    assert kvs[1]._layout_epoch != epoch and kvs[1].info["offset"] == [5, 5]
    before = [[_segments(kv, l) for l in range(L)] for kv in kvs]
    inputs = _step_inputs(g, 2)
    outs = [batch.update_attend(*inputs[l], l) for l in range(L)]
    _oracle_step(kvs, before, inputs, outs, "after slice + tighten")
    assert kvs[0].info["offset"] == [1, 1] and kvs[1].info["offset"] == [6, 6]
    # a member alone afterwards, then retired: the batch leaves it untouched
    single = kvs[0].update_attend(inputs[0][0][:1], inputs[0][1][:1], inputs[0][2][:1], 0)
    assert single.shape == (HKV, G_, D_) and kvs[0].info["offset"] == [2, 1]
    kvs[0].slice(kvs[0].get_seq_length() - 2)
    batch.retire(0)
    k0 = kvs[0].key_cache[0].clone()
    seen0 = kvs[0]._seen_tokens
    before = [[_segments(kv, l) for l in range(L)] for kv in kvs]
    inputs = _step_inputs(g, 2)
    outs = [batch.update_attend(*inputs[l], l) for l in range(L)]
    assert all(bool((o[0] == 0).all()) for o in outs)
    assert torch.equal(kvs[0].key_cache[0], k0) and kvs[0]._seen_tokens == seen0 and kvs[0].info["offset"] == [0, 0]
    _oracle_step(kvs[1:], before[1:], [(q[1:], k[1:], v[1:]) for q, k, v in inputs], [o[1:] for o in outs], "member 0 retired")


def test_member_slack_grows_inside_the_batch():
    from kvzip_amd.kvcache import CacheBatch
    kvs = [_evict_cache(300, 3, slack=2), _evict_cache(200, 4, slack=16)]
    batch = CacheBatch(kvs)
    g = torch.Generator().manual_seed(9)
    for step in range(4):          # the third step does not fit the slack of 2 any more
        before = [[_segments(kv, l) for l in range(L)] for kv in kvs]
        inputs = _step_inputs(g, 2)
        outs = [batch.update_attend(*inputs[l], l) for l in range(L)]
        _oracle_step(kvs, before, inputs, outs, f"slack/step{step}")
    assert kvs[0].slack > 2 and kvs[1].slack == 16
    assert kvs[0].info["offset"] == [4, 4] and kvs[1].info["offset"] == [4, 4]
