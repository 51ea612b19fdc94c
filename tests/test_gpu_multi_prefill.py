"""GPU: the packed first step over several independent pruned caches (kvz_multi_prefill, CacheBatch.select_packed / first_step) - exact
probes (bit equality of the output and of both arenas, tests/multi_prefill_probes.py), a cache without positions, oracle parity on
random data, and parity with the per-cache path (update + prepare + attend) through real EvictCache objects."""
import dataclasses
import functools

import pytest
import torch

import attn_probes as ap
import kvzip_oracle as orc
import multi_prefill_probes as mpp
from conftest import check_attn
from test_gpu_multi_attn import D_, G_, HKV, L, _evict_cache, _segments, _step_inputs, knob

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}     # the project's bounds (tests/test_gpu_multi_attn.py, test_gpu_fork_attn.py)
# B = 3 caches of Hkv = 2 heads: a head of several key ranges beside a head of one wave tile, an EMPTY head (a dropped head of a
# head-level cache), edges of the 32-key wave tiles and of the 128-key chunk unit
LENS = [[3000, 37], [0, 129], [64, 255]]
OFFSETS = [0, 5, 1]
SLACK = 40
# run lengths: a cache without positions, n_b = 1, a run crossing the 32-key tile of its own new rows
RUNS = [[5, 0, 17], [17, 3, 1], [1, 0, 5], [33, 1, 0]]
GEOMS = [(7, 128), (4, 128), (1, 128), (20, 64), (4, 64), (1, 64)]


def _ops():
    from kvzip_amd import ops
    return ops


def _run(c):
    """One kvz_multi_prefill call on the case's tensors -> (out, arena_k, arena_v) as the device holds them afterwards."""
    ops = _ops()
    q, kn, vn = (t.to(DEV) for t in mpp.as_model_tensors(c))
    assert kn.stride(2) != kn.shape[3] or kn.shape[1] == 1      # (a transposed view, as the projection hands it over)
    ak, av = c.arena_k.to(DEV), c.arena_v.to(DEV)
    ks = [ak[r:r + n] for r, n in zip(c.row0, c.rows)]
    vs = [av[r:r + n] for r, n in zip(c.row0, c.rows)]
    table = ops.MultiTable(ks, vs, c.starts, c.lens, c.slack)
    q0, kn0, vn0 = q.clone(), kn.clone(), vn.clone()
    out = ops.multi_prefill(q, c.cu_q, table, c.offset, kn, vn, softmax_scale=c.scale)
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and torch.equal(kn, kn0) and torch.equal(vn, vn0), "a read-only input was written"
    return out.cpu(), ak.cpu(), av.cpu()


@functools.lru_cache(maxsize=None)
def _probe(kind, lens, offsets, lengths, G, D, dtype, seed):
    """(case, expected out, expected arenas): computed once, shared by the attn_items values (nobody writes to them)."""
    make = mpp.uniform_case if kind == "uniform" else mpp.weighted_case
    c = make([list(x) for x in lens], list(offsets), list(lengths), G, D, dtype, SLACK, seed=seed)
    return c, mpp.expected_out(c), mpp.expected_arenas(c)


def _frozen(x):
    return tuple(tuple(r) for r in x)


def _check_exact(name, c, want=None, arenas=None):
    out, ak, av = _run(c)
    want = mpp.expected_out(c) if want is None else want
    same, n = ap.bits_equal(out, want)
    worst = int(ap.steps(out, want).max()) if want.numel() else 0
    print(f"\nMULTI-PREFILL {name}: {n} of {want.numel()} outputs differ; worst {worst} steps")
    assert same, (name, n, worst)
    ek, ev = mpp.expected_arenas(c) if arenas is None else arenas
    assert ap.bits_equal(ak, ek)[0] and ap.bits_equal(av, ev)[0], (name, "arenas: only the new rows of every (cache, head) may change")
    return out


@pytest.mark.parametrize("items", [3, 16, None], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", GEOMS)
def test_probes_exact(G, D, dtype, items):
    """items 3: every segment's old rows are one key range; 16: the 3000-key segment is cut into many ranges while the 37-key one is
    one; default: one block per CU.  G = 20: a position's rows straddle row tiles and 64-row groups."""
    with knob("attn_items", items):
        for i, lengths in enumerate(RUNS):
            for kind in ("uniform", "weighted"):
                c, want, arenas = _probe(kind, _frozen(LENS), tuple(OFFSETS), tuple(lengths), G, D, dtype, 10 * G + i)
                _check_exact(f"{kind} G{G} D{D} {dtype} items {items} runs {lengths}", c, want, arenas)


@pytest.mark.parametrize("items", [3, 16, None], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_row_group_edges(kind, items):
    """A run of exactly 128 rows (two full groups of four row tiles) and one of 70 rows (a group of one tile with 6 rows in it)."""
    with knob("attn_items", items):
        c, want, arenas = _probe(kind, _frozen(LENS), tuple(OFFSETS), (32, 1, 0), 4, 128, torch.float16, 21)
        _check_exact(f"{kind} 128 rows items {items}", c, want, arenas)
        c, want, arenas = _probe(kind, _frozen(LENS), tuple(OFFSETS), (10, 0, 3), 7, 64, torch.bfloat16, 22)
        _check_exact(f"{kind} 70 rows items {items}", c, want, arenas)


@pytest.mark.parametrize("items", [3, 16, None], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_chunk_unit_against_the_first_new_row(kind, items):
    """Base lengths 127 / 128 / 129 with offset 0: the last old key sits just below, on and just above the 128-key chunk unit, and
    the first new row follows it."""
    lens = ((127, 128), (129, 127), (128, 129))
    with knob("attn_items", items):
        for G, D, dtype in ((7, 128, torch.float16), (4, 64, torch.bfloat16)):
            c, want, arenas = _probe(kind, lens, (0, 0, 0), (3, 17, 1), G, D, dtype, 31)
            _check_exact(f"{kind} 127/128/129 G{G} D{D} items {items}", c, want, arenas)


def _without(c, b):
    """The same case with cache b's positions taken out of the packing (its rows of q, k_new and v_new removed)."""
    keep = [i for i in range(c.cu_q[-1]) if not c.cu_q[b] <= i < c.cu_q[b + 1]]
    lengths = c.lengths
    lengths[b] = 0
    return dataclasses.replace(c, q=c.q[:, keep].contiguous(), k_new=c.k_new[:, keep].contiguous(), v_new=c.v_new[:, keep].contiguous(),
                               cu_q=mpp._cu(lengths))


@pytest.mark.parametrize("items", [3, 16, None], ids=["items3", "items16", "default"])
@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_cache_without_positions(kind, items):
    """Cache 1 at n_b = 0: its rows of both arenas are byte-identical to before (the whole arenas are compared), and the other two
    caches give the bits they give when all three take part."""
    full, want, arenas = _probe(kind, _frozen(LENS), tuple(OFFSETS), (5, 3, 17), 7, 128, torch.float16, 41)
    part = _without(full, 1)
    assert part.cu_q == [0, 5, 5, 22]
    with knob("attn_items", items):
        a = _check_exact(f"{kind} all take part items {items}", full, want, arenas)
        out, ak, av = _run(part)
    ek, ev = mpp.expected_arenas(part)
    assert ap.bits_equal(ak, ek)[0] and ap.bits_equal(av, ev)[0]
    lo, hi = part.row0[1], part.row0[1] + part.rows[1]
    assert ap.bits_equal(ak[lo:hi], part.arena_k[lo:hi])[0] and ap.bits_equal(av[lo:hi], part.arena_v[lo:hi])[0]
    assert ap.bits_equal(out[:, 0:5], a[:, 0:5])[0] and ap.bits_equal(out[:, 5:22], a[:, 8:25])[0]
    assert ap.bits_equal(out, mpp.expected_out(part))[0]


def test_empty_packing_is_a_no_op():
    c = mpp.uniform_case(LENS, OFFSETS, [0, 0, 0], 7, 128, torch.float16, SLACK)
    out, ak, av = _run(c)
    assert out.numel() == 0 and ap.bits_equal(ak, c.arena_k)[0] and ap.bits_equal(av, c.arena_v)[0]


# ---- oracle parity on random data ----------------------------------------------------------------------------------------------------
def _check_oracle(name, c):
    out, ak, av = _run(c)
    ek, ev = mpp.expected_arenas(c)
    assert ap.bits_equal(ak, ek)[0] and ap.bits_equal(av, ev)[0], (name, "appended rows")
    Hkv, T, G, D = c.q.shape
    for b, n_b in enumerate(c.lengths):
        if n_b == 0:
            continue
        q, kk, vv, starts, lens = mpp.concat_for_oracle(c, b)
        want = orc.varlen_attn(q, kk, vv, starts, lens, n_b)
        got = out[:, c.cu_q[b]:c.cu_q[b + 1]].reshape(Hkv * n_b, G, D)
        check_attn(f"multi-prefill/random/{name}/b{b}", got, want, TOL[c.dtype], ulp_of=c.dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_oracle_parity_random(dtype):
    g = torch.Generator().manual_seed(11)
    # B = 1; B = 4 with very different caches (and one without positions); the limit B * Hkv = 128 with lengths <= 200
    _check_oracle(f"B1/{dtype}", mpp.random_case([[5, 3000, 129, 700]], [2], [19], 7, 128, dtype, slack=48, seed=1))
    _check_oracle(f"B4/{dtype}", mpp.random_case([[2500, 31], [0, 640], [129, 128], [1, 77]], [0, 3, 1, 7], [16, 3, 0, 40], 7, 128, dtype,
                                                 slack=48, seed=2))
    lens = torch.randint(0, 201, (16, 8), generator=g).tolist()
    offs = torch.randint(0, 6, (16,), generator=g).tolist()
    runs = torch.randint(0, 7, (16,), generator=g).tolist()
    _check_oracle(f"B16xHkv8/{dtype}", mpp.random_case(lens, offs, runs, 4, 64, dtype, slack=12, seed=3))
    with knob("attn_items", 16):
        _check_oracle(f"B16xHkv8/items16/{dtype}", mpp.random_case(lens, offs, runs, 20, 128, dtype, slack=12, seed=4))


# ---- CacheBatch.first_step against the per-cache path --------------------------------------------------------------------------------
def _first_inputs(g, T, dtype=torch.float16):
    """Per layer (query [1, H, T, D], key, value [1, Hkv, T, D]) as the attention layer hands them over (transposed views)."""
    mk = lambda h: torch.randn(1, T, h, D_, generator=g).to(dtype).to(DEV).transpose(1, 2)  # noqa: E731
    return [(mk(HKV * G_), mk(HKV), mk(HKV)) for _ in range(L)]


def _alone_first_step(kv, q, k, v, l, scale=None):
    """What attn.py does for ONE pruned cache with q_len > 1: update, prepare, attend -> [Hkv * q_len, G, D]."""
    kc, vc = kv.update(k, v, l)
    qq, kk, vv, info = kv.prepare(q.contiguous(), kc, vc, l)
    return kv.attend(qq, kk, vv, info, causal=True, softmax_scale=scale)


def _same_state(kvs, alone, what):
    for a, b in zip(kvs, alone):
        assert a.info["offset"] == b.info["offset"] and a._seen_tokens == b._seen_tokens, what
        assert a.get_seq_length() == b.get_seq_length() and a.slack == b.slack and a._mem() == b._mem(), what
        for l in range(L):
            assert torch.equal(a.info["seg_start"][l], b.info["seg_start"][l]), what
            for (ka, va), (kb, vb) in zip(_segments(a, l), _segments(b, l)):
                assert ap.bits_equal(ka, kb)[0] and ap.bits_equal(va, vb)[0], ("rows", what, l)


def _packed_vs_alone(kvs, alone, order, lengths, seed, name):
    """select_packed + first_step per layer on the batch against update / prepare / attend on the clones; then two batched decode
    steps against the clones stepped alone; then slice everything back."""
    from kvzip_amd.kvcache import CacheBatch
    g = torch.Generator().manual_seed(seed)
    seen0 = [kv.get_seq_length() for kv in kvs]
    batch = CacheBatch(kvs)
    T = sum(lengths)
    inputs = _first_inputs(g, T)
    batch.select_packed(order, lengths)
    for l, (q, k, v) in enumerate(inputs):
        got = batch.first_step(q, k, v, l)
        assert got.shape == (HKV, T, G_, D_)
        c0 = 0
        for b, n in zip(order, lengths):
            if n:
                want = _alone_first_step(alone[b], q[:, :, c0:c0 + n], k[:, :, c0:c0 + n], v[:, :, c0:c0 + n], l)
                check_attn(f"multi-prefill/{name}/l{l}/member{b}", got[:, c0:c0 + n].reshape(HKV * n, G_, D_), want, TOL[torch.float16],
                           ulp_of=torch.float16)
            c0 += n
    assert batch._packed is None                                   # cleared after the last layer
    _same_state(kvs, alone, name)
    for step in range(2):
        step_in = _step_inputs(g, len(kvs))
        for l, (q, k, v) in enumerate(step_in):
            got = batch.update_attend(q, k, v, l)
            for b in range(len(kvs)):
                want = alone[b].update_attend(q[b:b + 1], k[b:b + 1], v[b:b + 1], l)
                check_attn(f"multi-prefill/{name}/decode{step}/l{l}/member{b}", got[b], want, TOL[torch.float16], ulp_of=torch.float16)
        _same_state(kvs, alone, (name, "decode", step))
    for kv, a, s in zip(kvs, alone, seen0):
        kv.slice(s), a.slice(s)
    _same_state(kvs, alone, (name, "sliced"))
    assert all(kv.info["offset"] == [0] * L and kv.get_seq_length() == s for kv, s in zip(kvs, seen0))


@pytest.mark.parametrize("order,lengths", [([0, 1, 2], [5, 17, 40]), ([2, 0], [33, 1])], ids=["all", "two-of-three-reordered"])
def test_first_step_matches_the_per_cache_path(order, lengths):
    seeds = [(300, 1), (417, 2), (150, 3)]
    kvs = [_evict_cache(n, s, slack=64) for n, s in seeds]
    alone = [_evict_cache(n, s, slack=64) for n, s in seeds]      # the same caches again, stepped alone
    g = torch.Generator().manual_seed(7)
    for _ in range(2):             # member 1 starts two rows ahead: the offsets differ between the members
        for l, (q, k, v) in enumerate(_step_inputs(g, 1)):
            kvs[1].update_attend(q, k, v, l), alone[1].update_attend(q, k, v, l)
    _packed_vs_alone(kvs, alone, order, lengths, 8, "packed-vs-alone")
    # a member alone afterwards, as before
    q, k, v = _step_inputs(g, 1)[0]
    assert kvs[0].update_attend(q, k, v, 0).shape == (HKV, G_, D_) and kvs[0].info["offset"] == [1, 0]


def test_member_slack_grows_inside_first_step():
    """Member 0 has room for 4 appended rows and gets 9: it is re-laid out inside first_step (as its own update would), the table is
    rebuilt, and everything still agrees with the clones; a run that ends exactly at the slack does not grow it."""
    kvs = [_evict_cache(300, 5, slack=4), _evict_cache(200, 6, slack=16)]
    alone = [_evict_cache(300, 5, slack=4), _evict_cache(200, 6, slack=16)]
    _packed_vs_alone(kvs, alone, [0, 1], [9, 14], 9, "slack")
    assert kvs[0].slack > 4 and kvs[1].slack == 16
