"""GPU: the packed first step of a forked decode (kvz_fork_prefill_tail, ForkedCache.select_packed) - exact probes (bit equality,
tests/prefill_probes.py), the merge with the shared partial, the memory postcondition, oracle parity through ForkedCache, parity
with the per-branch path, and a stale fork."""
import types

import pytest
import torch

import attn_probes as ap
import kvzip_oracle as orc
import prefill_probes as pp
from conftest import check_attn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}     # the table of tests/test_gpu_fork_attn.py (test_first_step_matches_oracle)
CAP = 56
# (lengths, tail_len) of B = 3 branches: lengths from (1, 3, 5, 17, 0), tail lengths from (0, 1, 31, 32, 33); always one branch without
# positions, its tail pre-filled.  With G = 7 a token's rows straddle a 16-row tile, 5 x 7 = 35 rows are three row tiles, 17 tokens
# cross a 16-key boundary of the diagonal, 31 / 32 / 33 old rows cross a 32-key tile.
PACKS = [([5, 0, 17], [31, 33, 0]), ([17, 3, 0], [33, 32, 1]), ([1, 0, 5], [0, 31, 1]), ([3, 17, 0], [1, 31, 32])]
GEOMS = [(7, 128), (4, 128), (1, 128), (7, 64), (4, 64), (1, 64)]


def _ops():
    from kvzip_amd import ops
    return ops


def _run(c, inplace=False):
    """One kvz_fork_prefill_tail call on the case's tensors -> (out, and everything the device holds afterwards)."""
    ops = _ops()
    q, kn, vn = (t.to(DEV) for t in pp.as_model_tensors(c))
    assert kn.stride(2) != kn.shape[3] or kn.shape[1] == 1      # (a transposed view, as the projection hands it over)
    tk, tv = c.tail_k.to(DEV), c.tail_v.to(DEV)
    osh, lse = c.o_shared.to(DEV), c.lse_shared.to(DEV)
    q0, kn0, vn0 = q.clone(), kn.clone(), vn.clone()
    out = ops.fork_prefill_tail(q, c.cu_q, tk, tv, c.tail_len, kn, vn, osh, lse, softmax_scale=c.scale, out=osh if inplace else None)
    torch.cuda.synchronize()
    assert (out is osh) == inplace
    assert torch.equal(q, q0) and torch.equal(kn, kn0) and torch.equal(vn, vn0), "a read-only input was written"
    assert torch.equal(lse.cpu(), c.lse_shared), "lse_shared was written"
    if not inplace:
        assert ap.bits_equal(osh, c.o_shared)[0], "o_shared was written by an out-of-place call"
    return out.cpu(), tk.cpu(), tv.cpu()


def _check_exact(name, c, inplace=False):
    out, tk, tv = _run(c, inplace)
    want = pp.expected_out(c)
    same, n = ap.bits_equal(out, want)
    print(f"\nPREFILL {name}: {n} of {want.numel()} outputs differ; worst {int(ap.steps(out, want).max())} steps")
    assert same, (name, n, int(ap.steps(out, want).max()))
    etk, etv = pp.expected_tails(c)
    assert ap.bits_equal(tk, etk)[0] and ap.bits_equal(tv, etv)[0], (name, "tails: only rows t_b .. t_b + n_b - 1 may change")
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", GEOMS)
def test_uniform_probe_exact(G, D, dtype):
    for i, (lengths, tail_len) in enumerate(PACKS):
        c = pp.uniform_case(lengths, tail_len, G, D, dtype, CAP, seed=i)
        out = _check_exact(f"uniform G{G} D{D} {dtype} {lengths} {tail_len}", c, inplace=bool(i & 1))
        for b in range(3):   # the dim that holds the branch number: exactly b + 1 on every row of the branch
            assert bool((out[:, c.cu_q[b]:c.cu_q[b + 1], :, D - 1].float() == b + 1).all()), (b, "a row of another branch was seen")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("G,D", GEOMS)
def test_weighted_probe_exact(G, D, dtype):
    for i, (lengths, tail_len) in enumerate(PACKS):
        c = pp.weighted_case(lengths, tail_len, G, D, dtype, CAP, seed=i)
        _check_exact(f"weighted G{G} D{D} {dtype} {lengths} {tail_len}", c, inplace=bool(i & 1))


@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_one_branch_of_128_rows(kind):
    """G = 64, two tokens: 128 query rows of one (branch, head) are eight row tiles in two blocks; a token is four whole tiles."""
    make = pp.uniform_case if kind == "uniform" else pp.weighted_case
    _check_exact(f"{kind} G64", make([2, 0, 2], [31, 3, 0], 64, 128, torch.float16, CAP, Hkv=1, seed=3))
    _check_exact(f"{kind} G64 D64", make([2, 2, 0], [33, 0, 1], 64, 64, torch.bfloat16, CAP, Hkv=1, seed=4))


def test_more_branches_and_a_tail_of_several_tiles():
    """Sixteen branches (the limit), some of them empty, and old tails of several 32-key tiles with a query of several row-tile groups."""
    lengths = [3, 0, 1, 5, 2, 0, 17, 1, 1, 4, 0, 2, 6, 1, 3, 2]
    tail_len = [(7 * b) % 34 for b in range(16)]
    _check_exact("uniform B16", pp.uniform_case(lengths, tail_len, 4, 128, torch.float16, CAP, seed=5))
    _check_exact("weighted B16", pp.weighted_case(lengths, tail_len, 4, 64, torch.bfloat16, CAP, seed=5))
    _check_exact("uniform long", pp.uniform_case([40, 0, 9], [100, 3, 130], 7, 128, torch.bfloat16, 160, seed=6))   # 280 rows: 5 blocks
    _check_exact("weighted long", pp.weighted_case([40, 0, 9], [100, 3, 130], 7, 128, torch.float16, 160, seed=6))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", ["uniform", "weighted"])
def test_merge_with_the_shared_partial_exact(kind, dtype):
    """o_shared exactly representable, lse_shared such that both weights are powers of two: the merged result bit for bit, and the
    same bits whether `out` is o_shared or a buffer of its own."""
    make = pp.uniform_case if kind == "uniform" else pp.weighted_case
    for i, (G, D) in enumerate([(7, 128), (4, 64)]):
        lengths, tail_len = PACKS[i]
        c = pp.with_shared(make(lengths, tail_len, G, D, dtype, CAP, seed=i), seed=i)
        a = _check_exact(f"merge {kind} G{G} D{D} {dtype}", c, inplace=False)
        b = _check_exact(f"merge in place {kind} G{G} D{D} {dtype}", c, inplace=True)
        assert ap.bits_equal(a, b)[0]


def test_empty_packing_is_a_no_op():
    c = pp.uniform_case([0, 0, 0], [3, 0, 33], 7, 128, torch.float16, CAP)
    out, tk, tv = _run(c)
    assert out.numel() == 0 and ap.bits_equal(tk, c.tail_k)[0] and ap.bits_equal(tv, c.tail_v)[0]


# ---- through ForkedCache, against the oracle -----------------------------------------------------------------------------------------
def _evict_cache(lens, G, D, dtype, slack=64, seed=0):
    """A pruned slack-layout EvictCache of one layer with the given head lengths (the construction of tests/test_gpu_fork_attn.py:
    the score decides, head h keeps lens[h] - sink of N context rows)."""
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


def _packed_inputs(Hkv, G, D, T, dtype, g):
    """query [1, H, T, D], key / value [1, Hkv, T, D] as the attention layer produces them (transposed views of [1, T, heads, D])."""
    mk = lambda heads: torch.randn(1, T, heads, D, generator=g).to(dtype).to(DEV).transpose(1, 2)  # noqa: E731
    return mk(Hkv * G), mk(Hkv), mk(Hkv)


def _shared_rows(kv, lens):
    seg = kv.info["seg_start"][0].tolist()
    return ([kv.key_cache[0][seg[h]:seg[h] + lens[h]].cpu() for h in range(len(lens))],
            [kv.value_cache[0][seg[h]:seg[h] + lens[h]].cpu() for h in range(len(lens))])


def _oracle(shared, own_k, own_v, q_rows, n, G, D):
    """orc.varlen_attn on a branch's explicit concatenation: shared rows ++ its own rows (all of them, the last n being the queries'),
    bottom-right causal.  own_k / own_v [Hkv, rows, D]; q_rows [Hkv, n, G, D]."""
    sk, sv = shared
    Hkv = len(sk)
    ks, vs, starts, ln, acc = [], [], [], [], 0
    for h in range(Hkv):
        ks += [sk[h], own_k[h]]
        vs += [sv[h], own_v[h]]
        m = sk[h].shape[0] + own_k.shape[1]
        starts.append(acc); ln.append(m); acc += m
    return orc.varlen_attn(q_rows.reshape(Hkv * n, G, D), torch.cat(ks), torch.cat(vs), starts, ln, n, causal=True)


def _branch_rows(x, cu, i):
    """Rows of the i-th run of a packed [1, heads, T, D] tensor as [heads, n, D] on the host."""
    return x[0, :, cu[i]:cu[i + 1]].cpu()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("lens,G,D", [([4, 2500, 131, 640], 7, 128), ([4, 2500, 131, 640], 2, 64)], ids=["G7D128", "G2D64"])
def test_packed_first_step_matches_oracle_and_the_per_branch_path(lens, G, D, dtype):
    """fork(3), select_packed([2, 0, 1], [11, 3, 70]), one packed first_step; a second one on the non-empty tails; one decode step of all
    branches - every branch's rows against the oracle on its explicit concatenation.  The same inputs through select_branch +
    first_step per branch on a cache with the same rows: same results within the same tolerance, bit-identical tails."""
    Hkv = len(lens)
    kv, kv2 = _evict_cache(lens, G, D, dtype), _evict_cache(lens, G, D, dtype)
    shared = _shared_rows(kv, lens)
    before_k, before_v = kv.key_cache[0].clone(), kv.value_cache[0].clone()
    fork, ref = kv.fork(3, tail_capacity=8), kv2.fork(3, tail_capacity=8)      # (outgrown: the tails are re-allocated on the way)
    g = torch.Generator().manual_seed(G)
    own_k = {b: torch.zeros(Hkv, 0, D, dtype=dtype) for b in range(3)}
    own_v = {b: torch.zeros(Hkv, 0, D, dtype=dtype) for b in range(3)}
    for rnd, (branches, lengths) in enumerate((([2, 0, 1], [11, 3, 70]), ([1, 2, 0], [5, 33, 2]))):
        T = sum(lengths)
        cu = [sum(lengths[:i]) for i in range(len(lengths) + 1)]
        q, k, v = _packed_inputs(Hkv, G, D, T, dtype, g)
        fork.select_packed(branches, lengths)
        got = fork.first_step(q, k, v, 0).cpu()                                 # [Hkv, T, G, D]
        assert fork._packed is None                                             # (one layer: cleared after the last layer's call)
        assert got.shape == (Hkv, T, G, D)
        for i, (b, n) in enumerate(zip(branches, lengths)):
            own_k[b] = torch.cat([own_k[b], _branch_rows(k, cu, i)], dim=1)
            own_v[b] = torch.cat([own_v[b], _branch_rows(v, cu, i)], dim=1)
            q_rows = q[0, :, cu[i]:cu[i + 1]].cpu().reshape(Hkv, G, n, D).transpose(1, 2)          # [Hkv, n, G, D]
            want = _oracle(shared, own_k[b], own_v[b], q_rows, n, G, D)
            mine = got[:, cu[i]:cu[i + 1]].reshape(Hkv * n, G, D)
            check_attn(f"prefill/packed/G{G}D{D}/{dtype}/round{rnd}/b{b}", mine, want, TOL[dtype], ulp_of=dtype)
            # the per-branch path of today on the same rows
            ref.select_branch(b)
            sl = slice(cu[i], cu[i + 1])
            one = ref.first_step(q[:, :, sl], k[:, :, sl], v[:, :, sl], 0).cpu()                 # [Hkv, n, G, D]
            check_attn(f"prefill/packed-vs-per-branch/G{G}D{D}/{dtype}/round{rnd}/b{b}", mine, one.reshape(Hkv * n, G, D), TOL[dtype],
                       ulp_of=dtype)
        assert fork.tail_len[0] == ref.tail_len[0] == [own_k[b].shape[1] for b in range(3)]
        for b in range(3):
            t = fork.tail_len[0][b]
            assert torch.equal(fork.tail_k[0][b, :, :t].cpu(), own_k[b]) and torch.equal(fork.tail_v[0][b, :, :t].cpu(), own_v[b])
            assert torch.equal(fork.tail_k[0][b, :, :t], ref.tail_k[0][b, :, :t]) and torch.equal(fork.tail_v[0][b, :, :t], ref.tail_v[0][b, :, :t])
    assert fork.tail_len[0] == [5, 75, 44]
    # one decode step of all branches over shared ++ their tails
    q = torch.randn(3, Hkv * G, 1, D, generator=g).to(dtype).to(DEV)
    k = torch.randn(3, Hkv, 1, D, generator=g).to(dtype).to(DEV)
    v = torch.randn(3, Hkv, 1, D, generator=g).to(dtype).to(DEV)
    got = fork.update_attend(q, k, v, 0).cpu()
    for b in range(3):
        want = _oracle(shared, torch.cat([own_k[b], k[b].cpu()], dim=1), torch.cat([own_v[b], v[b].cpu()], dim=1),
                       q[b].cpu().view(Hkv, 1, G, D), 1, G, D)
        check_attn(f"prefill/decode-after-packed/G{G}D{D}/{dtype}/b{b}", got[b].reshape(Hkv, G, D), want, TOL[dtype], ulp_of=dtype)
    # the base cache is as it was, slack rows included
    assert kv.info["offset"] == [0]
    assert ap.bits_equal(kv.key_cache[0], before_k)[0] and ap.bits_equal(kv.value_cache[0], before_v)[0]


def test_stale_fork_raises():
    """After the base is re-laid out, a packed first_step raises as the other hooks do."""
    from kvzip_amd.ops import KvzError
    G, D, lens = 7, 128, [4, 300, 131, 64]
    kv = _evict_cache(lens, G, D, torch.float16, slack=4)
    fork = kv.fork(2)
    g = torch.Generator().manual_seed(0)
    q, k, v = _packed_inputs(4, G, D, 5, torch.float16, g)
    fork.select_packed([0, 1], [2, 3])
    fork.first_step(q, k, v, 0)
    kv._grow_slack(16)
    fork.select_packed([1, 0], [2, 3])
    with pytest.raises(KvzError, match="re-laid out"):
        fork.first_step(q, k, v, 0)
    assert fork.tail_len[0] == [2, 3]
    fork2 = kv.fork(2)                     # a new fork of the new layout works
    fork2.select_packed([1, 0], [2, 3])
    fork2.first_step(q, k, v, 0)
    assert fork2.tail_len[0] == [3, 2]
    with pytest.raises(KvzError, match="5 positions"):
        fork2.select_packed([0], [4])
        fork2.first_step(q, k, v, 0)
